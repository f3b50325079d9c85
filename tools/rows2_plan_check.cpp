// rows2_plan_check.cpp -- (check, host only) the host side of pulling out of a send layout,
// ompi-release_amd/csrc/rt/ddt_rows_plan.hpp, against its contract written out by brute force:
//   * move_send_direct_ok, the rule by which a sender publishes its layout instead of packing:
//     every clause on its own -- one run per block, not gap-free for the largest count, not in place,
//     no negative run displacement (nor a stride or an extent that reaches below the buffer), no
//     negative piece displacement, every piece below kSlot32Max packed bytes (the edge itself),
//     the run on both sides of MIN_RUN, MIN_RUN 0 = never;
//   * plan_rows2_multi: the pieces kept are those that hold bytes, in the caller's order; W is the
//     widest power of two <= 16 dividing, for EVERY kept piece, its length and on BOTH ends the first
//     byte, run length, stride and extent (a dense end: its base), tried width by width; the block
//     table starts at 0, is strictly monotone, gives every kept piece at least one block and its
//     share of the budget, and the kernel's walk over it touches every slot exactly once;
//   * the slot mapping the kernel applies (row_slot_off over row_end, the two fast divisions) on
//     both ends against a byte-by-byte enumeration of both layouts: slot q of a piece starts at the
//     memory offset of packed byte q * W and its W bytes are consecutive there; a dense end is one row.
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

// ---------------------------------------------------------------------------------- the rule
static bool want_ok(const SendShape &sh, const std::vector<size_t> &cnt, const std::vector<int64_t> *dsp, bool in_place,
                    int64_t min_run)
{
    if (sh.nruns != 1) return false;                      // one run per block
    size_t most = 0;
    for (size_t c : cnt) most = c > most ? c : most;
    const RowLay &l = sh.lay;
    // gap-free for `most` instances: the rows of an instance abut, and so do the instances
    const bool rows_abut = l.nblk <= 1 || l.stride == l.run;
    const bool inst_abut = most <= 1 || l.extent == l.nblk * l.run;
    if (rows_abut && inst_abut) return false;             // the plain call
    if (in_place) return false;
    if (l.disp < 0) return false;                         // first byte below the buffer
    if (l.nblk > 1 && l.stride < 0) return false;         // (a later row below it)
    if (most > 1 && l.extent < 0) return false;           // (a later instance below it)
    if (dsp)
        for (int64_t d : *dsp)
            if (d < 0) return false;
    for (size_t c : cnt) {
        // the piece's packed size below kSlot32Max, without overflow: c * size < kSlot32Max
        if (sh.size > 0 && c > (size_t)(kSlot32Max - 1) / (size_t)sh.size) return false;
    }
    if (min_run == 0) return false;                       // never
    return l.run >= min_run;
}

static void check_rule()
{
    static const int64_t runs[] = {1, 3, 8, 16, 64};
    static const int64_t nblks[] = {1, 2, 5};
    static const int64_t disps[] = {0, 8, -4};
    static const std::vector<size_t> counts[] = {{1}, {0, 0}, {2, 0, 1}, {1, 1, 1}, {7, 3}};
    for (int nruns = 1; nruns <= 3; ++nruns)
        for (int64_t run : runs)
            for (int64_t nblk : nblks)
                for (int64_t disp : disps)
                    for (int st = 0; st < 4; ++st)
                        for (int ex = 0; ex < 3; ++ex)
                            for (const auto &cnt : counts)
                                for (int dk = 0; dk < 3; ++dk)
                                    for (int ip = 0; ip < 2; ++ip) {
                                        const int64_t stride = st == 0 ? run : st == 1 ? run + 1 : st == 2 ? 2 * run : -2 * run;
                                        const int64_t tight = nblk * run, span = (nblk - 1) * (stride < 0 ? -stride : stride) + run;
                                        const int64_t extent = ex == 0 ? tight : ex == 1 ? span + 8 : -span;
                                        SendShape sh{nruns, RowLay{nblk, disp, run, stride, extent}, nblk * run};
                                        std::vector<int64_t> dsp(cnt.size(), 16);
                                        if (dk == 2) dsp.back() = -16;
                                        for (int64_t mr : {(int64_t)0, (int64_t)1, run - 1, run, run + 1}) {
                                            if (mr < 0) continue;
                                            ++checked;
                                            const bool got = move_send_direct_ok(sh, cnt.data(), dk ? dsp.data() : nullptr, (int)cnt.size(),
                                                                                 ip != 0, mr);
                                            const bool want = want_ok(sh, cnt, dk ? &dsp : nullptr, ip != 0, mr);
                                            CHECK(got == want,
                                                  "rule: %d want %d (nruns %d run %lld nblk %lld disp %lld stride %lld extent %lld min_run %lld "
                                                  "in_place %d displs %d)",
                                                  got, want, nruns, (long long)run, (long long)nblk, (long long)disp, (long long)stride,
                                                  (long long)extent, (long long)mr, ip, dk);
                                        }
                                    }
    // the kSlot32Max edge: 2^20-byte instances; 4092 of them are exactly kSlot32Max bytes
    {
        const SendShape sh{1, RowLay{1 << 10, 0, 1 << 10, 2 << 10, 4 << 20}, (int64_t)1 << 20};
        const size_t at = (size_t)(kSlot32Max >> 20);
        CHECK((int64_t)at << 20 == kSlot32Max, "the edge is no whole number of instances");
        for (size_t c : {at - 1, at, at + 1, (size_t)1 << 44}) {
            const std::vector<size_t> cnt = {1, c, 2};
            ++checked;
            const bool got = move_send_direct_ok(sh, cnt.data(), nullptr, 3, false, 1);
            CHECK(got == (c < at) && got == want_ok(sh, cnt, nullptr, false, 1), "rule: %zu instances of 1 MiB: %d", c, got);
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
            return ((uintptr_t)base + (uintptr_t)l.disp) % (uintptr_t)w == 0 && l.run % w == 0 && l.stride % w == 0 && l.extent % w == 0;
        };
        for (const Row2Seg &g : segs) {
            if (g.len == 0) continue;
            ok = ok && g.len % (size_t)w == 0 && end_ok(g.s, g.src) && end_ok(dst, g.mem);
        }
        if (ok) return w;
    }
    return 1;
}

// memory offset (from the end's base) of every byte of the first `len` packed bytes, by walking the
// layout instance by instance, row by row, byte by byte
static std::vector<int64_t> enumerate(const RowLay &l, size_t len)
{
    std::vector<int64_t> off;
    off.reserve(len);
    if (l.nblk == 0) {
        for (size_t x = 0; x < len; ++x) off.push_back((int64_t)x);
        return off;
    }
    for (int64_t k = 0; off.size() < len; ++k)
        for (int64_t j = 0; j < l.nblk && off.size() < len; ++j)
            for (int64_t o = 0; o < l.run && off.size() < len; ++o) off.push_back(k * l.extent + j * l.stride + l.disp + o);
    return off;
}

template <int W> static int64_t slot_off(const RowLay &l, const RowEnd &e, uint32_t q)
{
    return l.nblk ? row_slot_off<W, true>(e, q) + l.disp : row_slot_off<W, false>(e, q);
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
    const std::vector<int64_t> off = enumerate(l, len);
    const RowEnd e = row_end(l, w);
    for (size_t q = 0; q < len / (size_t)w; ++q) {
        ++checked;
        const int64_t got = slot_off_w(w, l, e, (uint32_t)q);
        bool ok = got == off[q * (size_t)w];
        for (int b = 1; b < w && ok; ++b) ok = off[q * (size_t)w + (size_t)b] == got + b;
        if (!ok) {
            CHECK(false, "%s end: slot %zu (W %d) at %lld, the layout has byte %zu at %lld (run %lld stride %lld extent %lld nblk %lld)",
                  which, q, w, (long long)got, q * (size_t)w, (long long)off[q * (size_t)w], (long long)l.run, (long long)l.stride,
                  (long long)l.extent, (long long)l.nblk);
            return;
        }
    }
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
        if (segs[(size_t)i].len == 0) continue;  // empty pieces are skipped
        CHECK(nk < p.nseg && p.seg[nk] == i, "kept piece %d: index %d, want %d", nk, nk < p.nseg ? p.seg[nk] : -1, i);
        ++nk;
        total += segs[(size_t)i].len;
    }
    CHECK(p.nseg == nk && p.total == total, "%d pieces %zu bytes kept, want %d %zu", p.nseg, p.total, nk, total);
    if (p.nseg != nk) return;
    if (nk == 0) {
        CHECK(p.w != 0 && p.first_block[0] == 0, "an empty plan declines");
        return;
    }
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
    // the kernel's walk: block -> piece from first_block[], lanes x U slots per pass, the blocks looping
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

int main()
{
    check_rule();
    alignas(64) static char sm[4][8192], dm[4][8192];
    static const RowLay lays[] = {
        {0, 0, 0, 0, 0},          // dense: one row
        {37, 0, 12, 20, 732},     // vector(37, 3, 5) of floats: W = 4
        {9, 0, 256, 512, 4352},   // vector(9, 64, 128) of floats: W = 16
        {50, 0, 8, 800, 8},       // a column of doubles resized to one element: W = 8
        {11, 0, 3, 7, 77},        // 3-byte runs at stride 7: W = 1
        {10, 16, 32, 48, 480},    // a displaced run
        {10, 6, 2, 10, 100},      // W = 2 at best
        {10, 4, 16, 32, 320},     // the displacement lowers W to 4
        {1, 0, 48, 0, 64},        // one row per instance
    };
    static const size_t lens[] = {0, 1, 3, 4, 6, 8, 12, 16, 48, 100, 256, 1000, 1024, 2048};
    static const size_t caps[] = {1, 3, 64, 100000};
    const unsigned tpb = 4, u16 = 2, un = 3;
    const size_t nl = sizeof(lays) / sizeof(lays[0]);
    // every pair of source and destination layout (dense on either end, on both): two pieces whose
    // sources differ, every length, misalignments of either base, every budget
    for (size_t d = 0; d < nl; ++d)
        for (size_t a = 0; a < nl; ++a)
            for (size_t cap : caps)
                for (size_t l0 : lens)
                    for (size_t l1 : {(size_t)0, (size_t)16, (size_t)96, (size_t)1000})
                        for (int mis = 0; mis < 9; ++mis) {
                            const int ms = (mis % 3) * 4, md = (mis / 3) * 8 % 20;   // 0,4,8 x 0,8,16
                            std::vector<Row2Seg> segs;
                            segs.push_back(Row2Seg{sm[0], lays[a], dm[0], l0});
                            segs.push_back(Row2Seg{sm[1] + ms, lays[(a + d + 1) % nl], dm[1] + md, l1});
                            segs.push_back(Row2Seg{sm[2], lays[0], dm[2], l0 / 2});
                            check_plan(lays[d], segs, tpb, u16, un, cap, cap == 64 && mis == 0);
                        }
    // a full list, the real launch shape; and one piece more than a launch holds
    for (size_t d = 0; d < nl; ++d)
        for (size_t cap : {(size_t)8, (size_t)262144}) {
            std::vector<Row2Seg> segs;
            for (int i = 0; i < kRowsMaxSegs; ++i) {
                const RowLay &l = lays[(size_t)i % nl];
                const size_t unit = l.nblk ? (size_t)(l.run * l.nblk) : 16;
                const size_t len = i % 5 == 0 ? 0 : i % 7 == 1 ? unit : unit * (size_t)(1 + i * 37 % 11) * 64;
                segs.push_back(Row2Seg{(char *)((uintptr_t)0x100000000ull * (uintptr_t)(i + 1)), l,
                                       (char *)(0x10000000ull + (uintptr_t)i * 0x100000ull), len});
            }
            check_plan(lays[d], segs, 256, 4, 8, cap, false);
            segs.push_back(segs[1]);
            ++checked;
            CHECK(plan_rows2_multi(lays[d], segs.data(), (int)segs.size(), 1024, 2048, cap).w == 0,
                  "more pieces than a launch holds were planned");
        }
    // the 32-bit limits: the largest piece a sender may publish (one byte below kSlot32Max) is planned
    // at W = 1 on a dense destination; a dense piece of kSlot32Max bytes at W = 1 declines
    {
        std::vector<Row2Seg> segs;
        segs.push_back(Row2Seg{(char *)0x100000001ull, lays[4], (char *)0x200000000ull, (size_t)kSlot32Max - 1});
        ++checked;
        CHECK(plan_rows2_multi(lays[0], segs.data(), 1, 1024, 2048, 4096).w == 1, "the largest publishable piece is not planned");
        segs[0] = Row2Seg{(char *)0x100000001ull, lays[0], (char *)0x200000000ull, (size_t)kSlot32Max};
        ++checked;
        CHECK(plan_rows2_multi(lays[0], segs.data(), 1, 1024, 2048, 4096).w == 0, "a piece beyond 32-bit slots was planned");
    }
    std::printf("{\"checked\": %ld, \"mismatches\": %ld}\n", checked, fails);
    return fails ? 1 : 0;
}
