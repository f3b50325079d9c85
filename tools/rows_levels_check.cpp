// rows_levels_check.cpp -- (check, host only) row layouts of up to two levels, the host side of
// pulling through 3-D subarray layouts (ompi-release_amd/csrc/rt/ddt_rows_plan.hpp), against its
// contract written out by brute force:
//   * row_levels_view, the normal form: every table it accepts enumerates, byte by byte, the same
//     offsets in the same order as the (runs, nblk, stride, extent) table it was read from; the level
//     count is the one a restatement of the rules gives (a level of count 1 vanishes, an outer level
//     that continues the inner one merges into it, a level 0 that continues the run merges into the
//     run), each rule also on a table written by hand; what was rows before there were levels (one
//     run per block, one block of equally spaced runs) keeps its five values, and with max_levels 1
//     nothing else is rows; an unequal length, one displacement off by one and three levels give 0;
//   * the slot mapping (row_slot_off over row_end) for W = 16, 8, 4, 2, 1 and an end of 0, 1 and 2
//     levels against the byte-by-byte enumeration of the layout;
//   * move_send_direct_ok against a restatement of its clauses with the second level in each: the
//     gap-free test, a negative step1, n1 >= 2^32, size == n0 * n1 * run, a piece at kSlot32Max;
//   * plan_rows2_multi with two-level ends: W is the widest power of two every kept piece allows on
//     both ends (step1 among the bits), the blocks are dealt as before and the kernel's walk touches
//     every slot once, and the plan declines at the 32-bit limits (n1, the slots of a piece).
// Stand-alone, under the host sanitizers; prints one JSON line, exit status 1 on any mismatch.
//   make -C tools check
#include "../ompi-release_amd/csrc/rt/ddt_rows_plan.hpp"

#include <cstdio>
#include <vector>

using namespace mi355x;

static long fails, checked;
#define CHECK(c, ...)                          \
    do {                                       \
        if (!(c)) {                            \
            if (++fails <= 20) {               \
                std::fprintf(stderr, __VA_ARGS__); \
                std::fputc('\n', stderr);      \
            }                                  \
        }                                      \
    } while (0)

struct Table {
    std::vector<int64_t> disp, len;
    int64_t nblk, stride, extent;
};

// memory offsets of the first n packed bytes of a table: instance, block, run, byte
static std::vector<int64_t> enum_table(const Table &t, size_t n)
{
    std::vector<int64_t> off;
    for (int64_t k = 0; off.size() < n; ++k)
        for (int64_t j = 0; j < t.nblk && off.size() < n; ++j)
            for (size_t r = 0; r < t.disp.size() && off.size() < n; ++r)
                for (int64_t o = 0; o < t.len[r] && off.size() < n; ++o) off.push_back(k * t.extent + j * t.stride + t.disp[r] + o);
    return off;
}

// ... of a row layout: instance, group, row, byte; a dense end is one row
static std::vector<int64_t> enum_lay(const RowLay &l, size_t n)
{
    std::vector<int64_t> off;
    if (l.nblk == 0) {
        for (size_t x = 0; x < n; ++x) off.push_back((int64_t)x);
        return off;
    }
    for (int64_t k = 0; off.size() < n; ++k)
        for (int64_t g = 0; g < l.n1 && off.size() < n; ++g)
            for (int64_t j = 0; j < l.nblk && off.size() < n; ++j)
                for (int64_t o = 0; o < l.run && off.size() < n; ++o)
                    off.push_back(k * l.extent + g * l.step1 + j * l.stride + l.disp + o);
    return off;
}

// ---------------------------------------------------------------------------------- the normal form
// what was rows before there were levels
static bool old_row_view(const Table &t, RowLay *l)
{
    const size_t n = t.disp.size();
    *l = RowLay{t.nblk, t.disp[0], t.len[0], t.stride, t.extent};
    if (n == 1) return t.len[0] > 0;
    if (t.nblk != 1 || t.len[0] <= 0) return false;
    const int64_t step = t.disp[1] - t.disp[0];
    for (size_t r = 1; r < n; ++r)
        if (t.len[r] != t.len[0] || t.disp[r] - t.disp[r - 1] != step) return false;
    *l = RowLay{(int64_t)n, t.disp[0], t.len[0], step, t.extent};
    return true;
}

// the rules restated on the levels a table was generated from, innermost first: the levels left
struct Lv {
    int64_t n, step;
};
static std::vector<Lv> normal_levels(std::vector<Lv> lv, int64_t *run)
{
    for (bool again = true; again;) {
        again = false;
        for (size_t i = 0; i < lv.size() && !again; ++i)
            if (lv[i].n == 1) {
                lv.erase(lv.begin() + (long)i);
                again = true;
            }
        for (size_t i = 0; i + 1 < lv.size() && !again; ++i)
            if (lv[i + 1].step == lv[i].n * lv[i].step) {
                lv[i].n *= lv[i + 1].n;
                lv.erase(lv.begin() + (long)i + 1);
                again = true;
            }
        if (!again && !lv.empty() && lv[0].step == *run) {
            *run *= lv[0].n;
            lv.erase(lv.begin());
            again = true;
        }
    }
    return lv;
}

static bool same5(const RowLay &a, const RowLay &b)
{
    return a.nblk == b.nblk && a.disp == b.disp && a.run == b.run && a.stride == b.stride && a.extent == b.extent;
}

static int view(const Table &t, RowLay *l, int max_levels = 2)
{
    return row_levels_view(t.disp.data(), t.len.data(), t.disp.size(), t.nblk, t.stride, t.extent, l, max_levels);
}

static void check_table(const Table &t, const std::vector<Lv> &gen, int64_t run, const char *what)
{
    ++checked;
    RowLay got, old;
    const int lev = view(t, &got);
    const bool was = old_row_view(t, &old);
    std::vector<Lv> left = gen;
    int64_t nrun = run;
    int want;
    if (was) want = 1;
    else {
        left = normal_levels(gen, &nrun);
        want = left.size() > 2 ? 0 : left.empty() ? 1 : (int)left.size();
    }
    CHECK(lev == want, "%s: %d levels, want %d (p %lld a %lld m %lld b %lld nblk %lld stride %lld run %lld)", what, lev, want,
          (long long)gen[0].n, (long long)gen[0].step, (long long)gen[1].n, (long long)gen[1].step, (long long)t.nblk,
          (long long)t.stride, (long long)run);
    RowLay one;
    const int lev1 = view(t, &one, 1);
    CHECK(lev1 == (was ? 1 : 0) && (!was || (same5(one, old) && one.n1 == 1)), "%s: max_levels 1 reads %d, rows before: %d", what,
          lev1, (int)was);
    if (lev != want || lev == 0) return;
    if (was) {
        CHECK(same5(got, old) && got.n1 == 1 && got.step1 == 0, "%s: a layout that was rows changed its five values", what);
    } else {
        const RowLay exp = left.empty() ? RowLay{1, t.disp[0], nrun, 0, t.extent}
                           : left.size() == 1
                               ? RowLay{left[0].n, t.disp[0], nrun, left[0].step, t.extent}
                               : RowLay{left[0].n, t.disp[0], nrun, left[0].step, t.extent, left[1].n, left[1].step};
        CHECK(same5(got, exp) && got.n1 == exp.n1 && got.step1 == exp.step1,
              "%s: normal form {%lld %lld %lld %lld %lld | %lld %lld}, want {%lld %lld %lld %lld %lld | %lld %lld}", what,
              (long long)got.nblk, (long long)got.disp, (long long)got.run, (long long)got.stride, (long long)got.extent,
              (long long)got.n1, (long long)got.step1, (long long)exp.nblk, (long long)exp.disp, (long long)exp.run,
              (long long)exp.stride, (long long)exp.extent, (long long)exp.n1, (long long)exp.step1);
    }
    CHECK(row_levels(got) == lev, "%s: row_levels of the normal form says %d, the view %d", what, row_levels(got), lev);
    int64_t inst = 0;
    for (int64_t x : t.len) inst += x;
    inst *= t.nblk;
    const size_t n = (size_t)(2 * inst + inst / 2 + 1);  // two instances and the stream ending inside the third
    const std::vector<int64_t> a = enum_table(t, n), b = enum_lay(got, n);
    bool same = a.size() == b.size();
    for (size_t i = 0; same && i < a.size(); ++i) same = a[i] == b[i];
    CHECK(same, "%s: the normal form enumerates other bytes than the table (p %lld a %lld m %lld b %lld nblk %lld stride %lld)", what,
          (long long)gen[0].n, (long long)gen[0].step, (long long)gen[1].n, (long long)gen[1].step, (long long)t.nblk,
          (long long)t.stride);
}

static Table make_table(int64_t d0, int64_t run, int64_t p, int64_t a, int64_t m, int64_t b, int64_t nblk, int64_t stride,
                        int64_t extent)
{
    Table t;
    for (int64_t r = 0; r < p * m; ++r) {
        t.disp.push_back(d0 + (r % p) * a + (r / p) * b);
        t.len.push_back(run);
    }
    t.nblk = nblk;
    t.stride = stride;
    t.extent = extent;
    return t;
}

static void check_normal_form()
{
    static const int64_t runs[] = {3, 4, 16, 48};
    static const int64_t ps[] = {1, 2, 3, 4}, ms[] = {1, 2, 3, 5}, nblks[] = {1, 2, 3};
    for (int64_t run : runs)
        for (int64_t p : ps)
            for (int64_t m : ms)
                for (int64_t nblk : nblks)
                    for (int ak = 0; ak < 3; ++ak)
                        for (int bk = 0; bk < 4; ++bk)
                            for (int sk = 0; sk < 4; ++sk)
                                for (int64_t d0 : {(int64_t)0, (int64_t)8}) {
                                    const int64_t a = ak == 0 ? run : ak == 1 ? run + 4 : 5 * run;
                                    const int64_t b = bk == 0 ? p * a : bk == 1 ? p * a + 8 : bk == 2 ? 7 * p * a : -(p * a + 8);
                                    const int64_t span = p * m * (b < 0 ? -b : b) + p * a;
                                    const int64_t stride = sk == 0 ? m * b : sk == 1 ? m * b + 16 : sk == 2 ? 3 * span : p * a;
                                    const int64_t extent = nblk * 4 * span + 32;
                                    const Table t = make_table(d0, run, p, a, m, b, nblk, stride, extent);
                                    // (the steps of a level of count 1 are never read: any value must do)
                                    check_table(t, {{p, p > 1 ? a : 12345}, {m, m > 1 ? b : -777}, {nblk, stride}}, run, "sweep");
                                    // one displacement off by one, one length unequal
                                    if (p * m >= 3) {
                                        Table u = t;
                                        u.disp[(size_t)(p * m - 1)] += 1;
                                        RowLay l;
                                        ++checked;
                                        CHECK(view(u, &l) == 0, "a table with one displacement off by one is rows");
                                        u = t;
                                        u.len[(size_t)(p * m / 2)] += 1;
                                        ++checked;
                                        CHECK(view(u, &l) == 0, "a table with one unequal length is rows");
                                    }
                                }
    // each rule on a table written by hand
    RowLay l;
    {   // rows in groups, several runs per block: 3 rows of 48 B at 80 B, 5 blocks at 400 B
        const Table t = make_table(0, 48, 3, 80, 1, 0, 5, 400, 2000);
        ++checked;
        CHECK(view(t, &l) == 2 && l.nblk == 3 && l.run == 48 && l.stride == 80 && l.n1 == 5 && l.step1 == 400 && l.extent == 2000 &&
                  l.disp == 0, "sub16 is not two levels");
        ++checked;
        CHECK(view(t, &l, 1) == 0, "sub16 is rows under max_levels 1");
    }
    {   // the same bytes as ONE block of 15 unrolled runs
        const Table t = make_table(0, 48, 3, 80, 5, 400, 1, 0, 2000);
        ++checked;
        CHECK(view(t, &l) == 2 && l.nblk == 3 && l.stride == 80 && l.n1 == 5 && l.step1 == 400, "the unrolled sub16 is not two levels");
    }
    {   // an outer level that continues the inner one: 3 rows at 80 B, 5 groups at 240 B = 15 rows
        const Table t = make_table(0, 48, 3, 80, 1, 0, 5, 240, 2000);
        ++checked;
        CHECK(view(t, &l) == 1 && l.nblk == 15 && l.run == 48 && l.stride == 80 && l.n1 == 1 && l.step1 == 0, "merge is not 15 rows");
    }
    {   // a level 0 that continues the run: 3 runs of 16 B abutting, 5 blocks at 100 B, 2 groups ... one level
        const Table t = make_table(4, 16, 3, 16, 1, 0, 5, 100, 1000);
        ++checked;
        CHECK(view(t, &l) == 1 && l.nblk == 5 && l.run == 48 && l.stride == 100 && l.disp == 4 && l.n1 == 1, "abutting runs did not merge");
    }
    {   // ... which makes room for a level above: abutting runs, then two levels
        const Table t = make_table(0, 16, 2, 16, 3, 100, 4, 1000, 8000);
        ++checked;
        CHECK(view(t, &l) == 2 && l.run == 32 && l.nblk == 3 && l.stride == 100 && l.n1 == 4 && l.step1 == 1000, "run merge, then two levels");
    }
    {   // three levels that do not merge
        const Table t = make_table(0, 16, 2, 32, 3, 100, 2, 1000, 8000);
        ++checked;
        CHECK(view(t, &l) == 0, "three levels are rows");
    }
    {   // everything abuts: one row per instance
        const Table t = make_table(0, 16, 2, 16, 3, 32, 2, 96, 500);
        ++checked;
        CHECK(view(t, &l) == 1 && l.nblk == 1 && l.run == 192 && l.n1 == 1 && l.extent == 500, "a gap-free block is not one row");
    }
    {   // what was rows stays: one run per block with abutting rows keeps its rows; a column stays a column
        const Table t = make_table(8, 16, 1, 0, 1, 0, 7, 16, 200);
        ++checked;
        CHECK(view(t, &l) == 1 && l.nblk == 7 && l.run == 16 && l.stride == 16 && l.disp == 8, "one run per block changed");
        const Table c = make_table(0, 8, 1, 0, 50, 800, 1, 0, 8);
        ++checked;
        CHECK(view(c, &l) == 1 && l.nblk == 50 && l.run == 8 && l.stride == 800 && l.extent == 8, "a column changed");
    }
}

// ---------------------------------------------------------------------------------- the slot mapping
template <int W> static int64_t slot_off(const RowLay &l, const RowEnd &e, uint32_t q)
{
    switch (row_levels(l)) {
    case 2: return row_slot_off<W, 2>(e, q) + l.disp;
    case 1: return row_slot_off<W, 1>(e, q) + l.disp;
    default: return row_slot_off<W, 0>(e, q);
    }
}

static int64_t slot_off_w(int w, const RowLay &l, const RowEnd &e, uint32_t q)
{
    switch (w) {
    case 16: return slot_off<16>(l, e, q);
    case 8: return slot_off<8>(l, e, q);
    case 4: return slot_off<4>(l, e, q);
    case 2: return slot_off<2>(l, e, q);
    default: return slot_off<1>(l, e, q);
    }
}

static void check_mapping(const RowLay &l, int w, size_t len, const char *which)
{
    const std::vector<int64_t> off = enum_lay(l, len);
    const RowEnd e = row_end(l, w);
    for (size_t q = 0; q < len / (size_t)w; ++q) {
        ++checked;
        const int64_t got = slot_off_w(w, l, e, (uint32_t)q);
        bool ok = got == off[q * (size_t)w];
        for (int b = 1; b < w && ok; ++b) ok = off[q * (size_t)w + (size_t)b] == got + b;
        if (!ok) {
            CHECK(false, "%s end: slot %zu (W %d) at %lld, the layout has byte %zu at %lld (run %lld n0 %lld step0 %lld n1 %lld step1 %lld)",
                  which, q, w, (long long)got, q * (size_t)w, (long long)off[q * (size_t)w], (long long)l.run, (long long)l.nblk,
                  (long long)l.stride, (long long)l.n1, (long long)l.step1);
            return;
        }
    }
}

static const RowLay kLays[] = {
    {0, 0, 0, 0, 0},                  // dense
    {37, 0, 12, 20, 732},             // one level, W = 4
    {9, 0, 256, 512, 4352},           // one level, W = 16
    {50, 0, 8, 800, 8},               // a column of doubles, W = 8
    {3, 0, 48, 80, 2000, 5, 400},     // sub16
    {3, 0, 8, 56, 8, 4, 224},         // sub8: pencils of doubles, C = 7
    {3, 0, 12, 20, 476, 7, 68},       // sub4
    {2, 0, 3, 7, 85, 5, 17},          // sub1
    {3, 6, 2, 10, 300, 4, 50},        // W = 2, displaced
    {2, 16, 32, 64, 1024, 3, 260},    // the second step lowers W to 4
    {1, 0, 16, 0, 640, 7, 48},        // one row per group
};
constexpr size_t kNLays = sizeof(kLays) / sizeof(kLays[0]);

static void check_mappings()
{
    for (const RowLay &l : kLays) {
        const uint64_t bits = l.nblk ? (uint64_t)l.run | (uint64_t)l.disp | (uint64_t)l.stride | (uint64_t)l.extent | (uint64_t)l.step1 : 0;
        const size_t inst = l.nblk ? (size_t)(l.run * l.nblk * l.n1) : 64;
        for (int w = 16; w >= 1; w >>= 1) {
            if (bits & (uint64_t)(w - 1)) continue;
            check_mapping(l, w, (3 * inst + inst / 2) / (size_t)w * (size_t)w, "an");
        }
    }
}

// ---------------------------------------------------------------------------------- the rule
static bool want_ok(const SendShape &sh, const std::vector<size_t> &cnt, const std::vector<int64_t> *dsp, bool in_place,
                    int64_t min_run)
{
    if (sh.nruns != 1) return false;                      // rows, not a run list
    size_t most = 0;
    for (size_t c : cnt) most = c > most ? c : most;
    const RowLay &l = sh.lay;
    if (l.n1 < 1 || l.nblk < 1) return false;
    // gap-free for `most` instances: rows abut, groups abut, instances abut
    const bool rows_abut = l.nblk <= 1 || l.stride == l.run;
    const bool grps_abut = l.n1 <= 1 || l.step1 == l.nblk * l.run;
    const bool inst_abut = most <= 1 || l.extent == l.n1 * l.nblk * l.run;
    if (rows_abut && grps_abut && inst_abut) return false;  // the plain call
    if (in_place) return false;
    if (l.disp < 0) return false;                         // first byte below the buffer
    if (l.nblk > 1 && l.stride < 0) return false;         // (a later row below it)
    if (l.n1 > 1 && l.step1 < 0) return false;            // (a later group below it)
    if (most > 1 && l.extent < 0) return false;           // (a later instance below it)
    if (l.n1 >> 32 || l.nblk >> 32 || l.run >> 32) return false;
    if (sh.size != l.n1 * l.nblk * l.run) return false;
    if (dsp)
        for (int64_t d : *dsp)
            if (d < 0) return false;
    for (size_t c : cnt)
        if (sh.size > 0 && c > (size_t)(kSlot32Max - 1) / (size_t)sh.size) return false;
    if (min_run == 0) return false;                       // never
    return l.run >= min_run;
}

static void check_rule()
{
    static const int64_t runs[] = {1, 8, 16};
    static const int64_t n0s[] = {1, 3}, n1s[] = {1, 2, 5};
    static const std::vector<size_t> counts[] = {{1}, {0, 0}, {2, 0, 1}, {7, 3}};
    for (int nruns = 1; nruns <= 2; ++nruns)
        for (int64_t run : runs)
            for (int64_t n0 : n0s)
                for (int64_t n1 : n1s)
                    for (int64_t disp : {(int64_t)0, (int64_t)-4})
                        for (int st = 0; st < 3; ++st)
                            for (int s1 = 0; s1 < 3; ++s1)
                                for (int ex = 0; ex < 3; ++ex)
                                    for (const auto &cnt : counts)
                                        for (int dk = 0; dk < 3; ++dk)
                                            for (int ip = 0; ip < 2; ++ip) {
                                                const int64_t stride = st == 0 ? run : st == 1 ? 2 * run : -2 * run;
                                                const int64_t step1 = s1 == 0 ? n0 * run : s1 == 1 ? 4 * n0 * run + 8 : -(4 * n0 * run);
                                                const int64_t tight = n1 * n0 * run;
                                                const int64_t extent = ex == 0 ? tight : ex == 1 ? 64 * tight : -64 * tight;
                                                SendShape sh{nruns, RowLay{n0, disp, run, stride, extent, n1, step1}, tight};
                                                std::vector<int64_t> dsp(cnt.size(), 16);
                                                if (dk == 2) dsp.back() = -16;
                                                for (int64_t mr : {(int64_t)0, (int64_t)1, run, run + 1}) {
                                                    ++checked;
                                                    const bool got = move_send_direct_ok(sh, cnt.data(), dk ? dsp.data() : nullptr,
                                                                                         (int)cnt.size(), ip != 0, mr);
                                                    const bool want = want_ok(sh, cnt, dk ? &dsp : nullptr, ip != 0, mr);
                                                    CHECK(got == want,
                                                          "rule: %d want %d (nruns %d run %lld n0 %lld step0 %lld n1 %lld step1 %lld disp %lld extent "
                                                          "%lld min_run %lld in_place %d displs %d)",
                                                          got, want, nruns, (long long)run, (long long)n0, (long long)stride, (long long)n1,
                                                          (long long)step1, (long long)disp, (long long)extent, (long long)mr, ip, dk);
                                                    CHECK(sh.levels() == (nruns != 1 ? 0 : n1 > 1 ? 2 : 1), "SendShape::levels %d", sh.levels());
                                                }
                                            }
    const std::vector<size_t> one = {1, 2};
    {   // the clauses of the second level, each on its own
        SendShape sh{1, RowLay{3, 0, 48, 80, 2000, 5, 400}, 720};
        ++checked;
        CHECK(move_send_direct_ok(sh, one.data(), nullptr, 2, false, 16), "sub16 is refused");
        sh.lay.step1 = -400;
        ++checked;
        CHECK(!move_send_direct_ok(sh, one.data(), nullptr, 2, false, 16) && !want_ok(sh, one, nullptr, false, 16), "a negative step1 passes");
        sh.lay.step1 = 400;
        sh.size = 144;  // (n0 * run: the size of the first group alone)
        ++checked;
        CHECK(!move_send_direct_ok(sh, one.data(), nullptr, 2, false, 16) && !want_ok(sh, one, nullptr, false, 16), "size != n0 * n1 * run passes");
        sh.lay.n1 = (int64_t)1 << 32;
        sh.lay.nblk = 1;
        sh.lay.run = 1;
        sh.size = (int64_t)1 << 32;
        const std::vector<size_t> none = {0, 0};
        ++checked;
        CHECK(!move_send_direct_ok(sh, none.data(), nullptr, 2, false, 1) && !want_ok(sh, none, nullptr, false, 1), "n1 = 2^32 passes");
        sh.lay.n1 = 0;
        sh.size = 0;
        ++checked;
        CHECK(!move_send_direct_ok(sh, none.data(), nullptr, 2, false, 1), "n1 = 0 passes");
    }
    {   // the kSlot32Max edge with both levels live: 2^20-byte instances, 4092 of them are the edge
        const SendShape sh{1, RowLay{1 << 5, 0, 1 << 10, 2 << 10, 16 << 20, 1 << 5, 1 << 17}, (int64_t)1 << 20};
        const size_t at = (size_t)(kSlot32Max >> 20);
        for (size_t c : {at - 1, at, at + 1, (size_t)1 << 44}) {
            const std::vector<size_t> cnt = {1, c, 2};
            ++checked;
            const bool got = move_send_direct_ok(sh, cnt.data(), nullptr, 3, false, 1);
            CHECK(got == (c < at) && got == want_ok(sh, cnt, nullptr, false, 1), "rule: %zu two-level instances of 1 MiB: %d", c, got);
        }
    }
}

// ---------------------------------------------------------------------------------- the plan
static int brute_w(const RowLay &dst, const std::vector<Row2Seg> &segs)
{
    for (int w = 16; w > 1; w >>= 1) {
        bool ok = true;
        auto end_ok = [&](const RowLay &l, const void *base) {
            if (l.nblk == 0) return (uintptr_t)base % (uintptr_t)w == 0;
            return ((uintptr_t)base + (uintptr_t)l.disp) % (uintptr_t)w == 0 && l.run % w == 0 && l.stride % w == 0 &&
                   l.step1 % w == 0 && l.extent % w == 0;
        };
        for (const Row2Seg &g : segs) {
            if (g.len == 0) continue;
            ok = ok && g.len % (size_t)w == 0 && end_ok(g.s, g.src) && end_ok(dst, g.mem);
        }
        if (ok) return w;
    }
    return 1;
}

static void check_plan(const RowLay &dst, const std::vector<Row2Seg> &segs, unsigned tpb, unsigned u16, unsigned un, size_t cap,
                       bool map)
{
    ++checked;
    const RowsMultiPlan p = plan_rows2_multi(dst, segs.data(), (int)segs.size(), tpb * u16, tpb * un, cap);
    const int w = brute_w(dst, segs);
    int nk = 0;
    size_t total = 0;
    for (int i = 0; i < (int)segs.size(); ++i) {
        if (segs[(size_t)i].len == 0) continue;
        CHECK(nk < p.nseg && p.seg[nk] == i, "kept piece %d: index %d, want %d", nk, nk < p.nseg ? p.seg[nk] : -1, i);
        ++nk;
        total += segs[(size_t)i].len;
    }
    CHECK(p.nseg == nk && p.total == total, "%d pieces %zu bytes kept, want %d %zu", p.nseg, p.total, nk, total);
    if (p.nseg != nk || nk == 0) return;
    CHECK(p.w == w, "W %d, want %d", p.w, w);
    if (p.w != w) return;
    CHECK(p.first_block[0] == 0, "first block %u", p.first_block[0]);
    const size_t per = (size_t)tpb * (w == 16 ? u16 : un);
    for (int s = 0; s < p.nseg; ++s) {
        const size_t len = segs[(size_t)p.seg[s]].len, nslots = len / (size_t)w;
        CHECK(p.first_block[s + 1] > p.first_block[s], "piece %d has no block", s);
        const size_t nb = p.first_block[s + 1] - p.first_block[s];
        const size_t want = (nslots + per - 1) / per;
        size_t share = 0;
        while (share * total < cap * len) ++share;
        const size_t lim = want < share ? want : share;
        CHECK(nb == (lim ? lim : 1), "piece %d: %zu blocks, want %zu", s, nb, lim ? lim : 1);
    }
    const unsigned U = w == 16 ? u16 : un;
    for (int s = 0; s < p.nseg; ++s) {
        std::vector<int> hit(segs[(size_t)p.seg[s]].len / (size_t)w, 0);
        for (unsigned blk = p.first_block[s]; blk < p.first_block[s + 1]; ++blk) {
            int sgi = 0;
            while (sgi + 1 < p.nseg && blk >= p.first_block[sgi + 1]) ++sgi;
            CHECK(sgi == s, "block %u finds piece %d, owned by %d", blk, sgi, s);
            const unsigned nb = p.first_block[s + 1] - p.first_block[s], b = blk - p.first_block[s];
            for (unsigned t = 0; t < tpb; ++t)
                for (uint64_t base = (uint64_t)b * per + t; base < hit.size(); base += (uint64_t)nb * per)
                    for (unsigned u = 0; u < U; ++u)
                        if (base + u * tpb < hit.size()) hit[base + u * tpb]++;
        }
        for (size_t i = 0; i < hit.size(); ++i)
            if (hit[i] != 1) {
                CHECK(false, "piece %d slot %zu moved %d times (W %d)", s, i, hit[i], w);
                break;
            }
    }
    if (!map) return;
    for (int s = 0; s < p.nseg; ++s) {
        const Row2Seg &g = segs[(size_t)p.seg[s]];
        check_mapping(g.s, w, g.len, "source");
        check_mapping(dst, w, g.len, "destination");
    }
}

static void check_plans()
{
    alignas(64) static char sm[4][8192], dm[4][8192];
    static const size_t lens[] = {0, 1, 3, 4, 6, 8, 12, 16, 48, 100, 720, 1000, 1024, 2048};
    static const size_t caps[] = {1, 3, 64, 100000};
    const unsigned tpb = 4, u16 = 2, un = 3;
    for (size_t d = 0; d < kNLays; ++d)
        for (size_t a = 0; a < kNLays; ++a)
            for (size_t cap : caps)
                for (size_t l0 : lens)
                    for (size_t l1 : {(size_t)0, (size_t)96, (size_t)1000})
                        for (int mis = 0; mis < 4; ++mis) {
                            const int ms = (mis % 2) * 4, md = (mis / 2) * 8;
                            std::vector<Row2Seg> segs;
                            segs.push_back(Row2Seg{sm[0], kLays[a], dm[0], l0});
                            segs.push_back(Row2Seg{sm[1] + ms, kLays[(a + d + 1) % kNLays], dm[1] + md, l1});
                            segs.push_back(Row2Seg{sm[2], kLays[0], dm[2], l0 / 2});
                            check_plan(kLays[d], segs, tpb, u16, un, cap, cap == 64 && mis == 0);
                        }
    // the real launch shape with a full list
    for (size_t d = 0; d < kNLays; ++d)
        for (size_t cap : {(size_t)8, (size_t)262144}) {
            std::vector<Row2Seg> segs;
            for (int i = 0; i < kRowsMaxSegs; ++i) {
                const RowLay &l = kLays[(size_t)i % kNLays];
                const size_t unit = l.nblk ? (size_t)(l.run * l.nblk * l.n1) : 16;
                const size_t len = i % 5 == 0 ? 0 : i % 7 == 1 ? unit : unit * (size_t)(1 + i * 37 % 11) * 16;
                segs.push_back(Row2Seg{(char *)((uintptr_t)0x100000000ull * (uintptr_t)(i + 1)), l,
                                       (char *)(0x10000000ull + (uintptr_t)i * 0x100000ull), len});
            }
            check_plan(kLays[d], segs, 256, 4, 8, cap, false);
        }
    // the 32-bit limits: the largest piece a sender may publish through two levels is planned at W = 1,
    // into a two-level destination too; n1 = 2^32 on either end declines; a dense piece of kSlot32Max
    // bytes into a two-level destination at W = 1 declines
    {
        std::vector<Row2Seg> segs;
        segs.push_back(Row2Seg{(char *)0x100000001ull, kLays[7], (char *)0x200000000ull, (size_t)kSlot32Max - 1});
        ++checked;
        CHECK(plan_rows2_multi(kLays[0], segs.data(), 1, 1024, 2048, 4096).w == 1, "the largest publishable two-level piece is not planned");
        ++checked;
        CHECK(plan_rows2_multi(kLays[6], segs.data(), 1, 1024, 2048, 4096).w == 1, "... nor into a two-level destination");
        RowLay big = kLays[4];
        big.n1 = (int64_t)1 << 32;
        segs[0] = Row2Seg{(char *)0x100000000ull, big, (char *)0x200000000ull, 4096};
        ++checked;
        CHECK(plan_rows2_multi(kLays[0], segs.data(), 1, 1024, 2048, 4096).w == 0, "a source of 2^32 groups was planned");
        segs[0] = Row2Seg{(char *)0x100000000ull, kLays[0], (char *)0x200000000ull, 4096};
        ++checked;
        CHECK(plan_rows2_multi(big, segs.data(), 1, 1024, 2048, 4096).w == 0, "a destination of 2^32 groups was planned");
        segs[0] = Row2Seg{(char *)0x100000001ull, kLays[0], (char *)0x200000000ull, (size_t)kSlot32Max};
        ++checked;
        CHECK(plan_rows2_multi(kLays[7], segs.data(), 1, 1024, 2048, 4096).w == 0, "a piece beyond 32-bit slots was planned");
    }
}

int main()
{
    check_normal_form();
    check_mappings();
    check_rule();
    check_plans();
    std::printf("{\"checked\": %ld, \"mismatches\": %ld}\n", checked, fails);
    return fails ? 1 : 0;
}
