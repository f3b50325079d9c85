// rows_plan_check.cpp -- (check, host only) the host side of the multi-segment row unpack,
// plan_rows_multi of ompi-release_amd/csrc/rt/ddt_rows_plan.hpp, against its contract written out
// by brute force, over layouts x piece lists x misalignments x block budgets:
//   * the pieces kept are those that hold bytes and whose packed source is not their memory base,
//     in the caller's order;
//   * W is the widest power of two <= 16 dividing, for EVERY kept piece, its packed address, its
//     first byte in memory, its length, and the run length, stride and extent (tried width by width);
//     a piece beyond the kernels' 32-bit slot arithmetic makes the plan decline (w = 0);
//   * every kept piece gets at least one block, never more than one per `per` slots, and when the
//     budget binds its share of it by bytes; the blocks of all pieces stay within cap + pieces;
//   * walking the grid as k_ddt_rows_multi does (block -> piece from first_block[], lanes x U slots
//     per pass, the piece's blocks looping) touches every slot of every kept piece exactly once and
//     nothing else.
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

struct Layout {
    int64_t run_disp, run_len, stride, extent, nblk;
};

static bool kept(const RowSeg &g) { return g.len != 0 && g.packed != g.mem; }

// the definition of W: try 16, 8, 4, 2 -- the first width dividing everything of every kept piece
static int brute_w(const Layout &l, const std::vector<RowSeg> &segs)
{
    for (int w = 16; w > 1; w >>= 1) {
        bool ok = l.run_len % w == 0 && l.stride % w == 0 && l.extent % w == 0;
        for (const RowSeg &g : segs) {
            if (!kept(g)) continue;
            ok = ok && (uintptr_t)g.packed % (uintptr_t)w == 0 && ((uintptr_t)g.mem + (uintptr_t)l.run_disp) % (uintptr_t)w == 0 &&
                 g.len % (size_t)w == 0;
        }
        if (ok) return w;
    }
    return 1;
}

static void check_plan(const Layout &l, const std::vector<RowSeg> &segs, unsigned tpb, unsigned u16, unsigned un, size_t cap,
                       bool walk)
{
    ++checked;
    const RowsMultiPlan p = plan_rows_multi(l.stride, l.extent, l.nblk, l.run_disp, l.run_len, segs.data(), (int)segs.size(),
                                            tpb * u16, tpb * un, cap);
    const int w = brute_w(l, segs);
    // the 32-bit limits (rows_width): last slot, rows, blocks per instance, slots per row
    bool fits = l.run_len > 0 && l.nblk < ((int64_t)1 << 32);
    for (const RowSeg &g : segs) {
        if (!kept(g)) continue;
        const int64_t last = (int64_t)g.len / w;
        fits = fits && last < kSlot32Max && last / (l.run_len / w) + 1 < ((int64_t)1 << 32);
    }
    if (!fits) {
        bool any = false;
        for (const RowSeg &g : segs) any = any || kept(g);
        CHECK(!any || p.w == 0, "a piece beyond 32-bit slots was planned (w %d)", p.w);
        return;
    }
    bool any_kept = false;
    for (const RowSeg &g : segs) any_kept = any_kept || kept(g);
    if (!any_kept) {  // nothing to launch: W means nothing
        CHECK(p.w != 0 && p.nseg == 0 && p.first_block[0] == 0 && p.total == 0, "an empty plan keeps %d pieces, w %d", p.nseg, p.w);
        return;
    }
    CHECK(p.w == w, "W %d, want %d (run %lld stride %lld extent %lld)", p.w, w, (long long)l.run_len, (long long)l.stride,
          (long long)l.extent);
    if (p.w != w) return;
    int nk = 0;
    size_t total = 0;
    for (int i = 0; i < (int)segs.size(); ++i) {
        if (!kept(segs[(size_t)i])) continue;
        CHECK(nk < p.nseg && p.seg[nk] == i, "kept piece %d: index %d, want %d", nk, nk < p.nseg ? p.seg[nk] : -1, i);
        ++nk;
        total += segs[(size_t)i].len;
    }
    CHECK(p.nseg == nk && p.total == total, "%d pieces %zu bytes kept, want %d %zu", p.nseg, p.total, nk, total);
    if (p.nseg != nk) return;
    CHECK(p.first_block[0] == 0, "first block %u", p.first_block[0]);
    const size_t per = (size_t)tpb * (w == 16 ? u16 : un);
    for (int s = 0; s < p.nseg; ++s) {
        const size_t len = segs[(size_t)p.seg[s]].len, nslots = len / (size_t)w;
        CHECK(p.first_block[s + 1] > p.first_block[s], "piece %d has no block", s);
        const size_t nb = p.first_block[s + 1] - p.first_block[s];
        const size_t want = (nslots + per - 1) / per;
        // its share of the budget by bytes, rounded up, by counting: the least k with k * total >= cap * len
        size_t share = 0;
        while (share * total < cap * len) ++share;
        const size_t lim = want < share ? want : share;
        CHECK(nb == (lim ? lim : 1), "piece %d: %zu blocks, want %zu (passes %zu, share %zu)", s, nb, lim ? lim : 1, want, share);
    }
    CHECK(p.first_block[p.nseg] <= cap + (size_t)p.nseg, "%u blocks for a budget of %zu and %d pieces", p.first_block[p.nseg], cap,
          p.nseg);
    if (!walk) return;
    // the kernel's walk
    const unsigned U = w == 16 ? u16 : un;
    std::vector<std::vector<int>> hit((size_t)p.nseg);
    for (int s = 0; s < p.nseg; ++s) hit[(size_t)s].assign(segs[(size_t)p.seg[s]].len / (size_t)w, 0);
    for (unsigned blk = 0; blk < p.first_block[p.nseg]; ++blk) {
        int sgi = 0;
        while (sgi + 1 < p.nseg && blk >= p.first_block[sgi + 1]) ++sgi;
        const unsigned nb = p.first_block[sgi + 1] - p.first_block[sgi], b = blk - p.first_block[sgi];
        const uint64_t nslots = hit[(size_t)sgi].size();
        for (unsigned t = 0; t < tpb; ++t)
            for (uint64_t base = (uint64_t)b * per + t; base < nslots; base += (uint64_t)nb * per)
                for (unsigned u = 0; u < U; ++u) {
                    const uint32_t i = (uint32_t)base + u * tpb;
                    if (i < nslots) hit[(size_t)sgi][i]++;
                }
    }
    for (int s = 0; s < p.nseg; ++s)
        for (size_t i = 0; i < hit[(size_t)s].size(); ++i)
            if (hit[(size_t)s][i] != 1) {
                CHECK(false, "piece %d slot %zu moved %d times (W %d, %u blocks)", s, i, hit[(size_t)s][i], w,
                      p.first_block[s + 1] - p.first_block[s]);
                break;
            }
}

int main()
{
    alignas(64) static char pk[8][4096], mm[8][4096];
    static const Layout layouts[] = {
        {0, 12, 20, 728, 37},      // vector(37, 3, 5) of floats: W = 4
        {0, 256, 512, 4352, 9},    // vector(9, 64, 128) of floats: W = 16
        {0, 8, 800, 8, 100},       // a column of doubles resized to one element: W = 8
        {0, 3, 7, 70, 10},         // 3-byte runs at stride 7: W = 1
        {16, 32, 48, 480, 10},     // a displaced run
        {6, 2, 10, 100, 10},       // W = 2 at best
        {4, 16, 32, 320, 10},      // the displacement lowers W to 4
        {0, 16, 24, 240, 10},      // the stride lowers it to 8
        {0, 16, 32, 328, 10},      // the extent lowers it to 8
    };
    static const size_t lens[] = {0, 1, 3, 4, 6, 8, 12, 16, 48, 100, 256, 1000, 1024, 4096};
    static const size_t caps[] = {1, 3, 7, 64, 100000};
    const unsigned tpb = 4, u16 = 2, un = 3;
    // one, two and three pieces: every length, misalignments of either side, every budget
    for (const Layout &l : layouts)
        for (size_t cap : caps)
            for (size_t l0 : lens)
                for (size_t l1 : lens)
                    for (int mis = 0; mis < 36; ++mis) {
                        const int mp = (mis % 6) * 3 % 17, mmem = (mis / 6) * 4 % 17;   // 0,3,6,9,12,15 x 0,4,8,12,16
                        std::vector<RowSeg> segs;
                        segs.push_back(RowSeg{pk[0], mm[0], l0});
                        segs.push_back(RowSeg{pk[1] + mp, mm[1] + mmem, l1});
                        check_plan(l, segs, tpb, u16, un, cap, true);
                        if (mis < 6) {
                            segs.push_back(RowSeg{mm[2] + mp, mm[2] + mp, 48});  // its own memory base: skipped
                            segs.push_back(RowSeg{pk[3] + 16, mm[3], l0 ? l0 * 2 : 16});
                            check_plan(l, segs, tpb, u16, un, cap, true);
                        }
                    }
    // a full list: one tiny piece beside large ones, zero-length ones between, the real launch shape
    for (const Layout &l : layouts)
        for (size_t cap : {(size_t)8, (size_t)256, (size_t)262144}) {
            std::vector<RowSeg> segs;
            for (int i = 0; i < kRowsMaxSegs; ++i) {
                const size_t unit = (size_t)l.run_len * (size_t)l.nblk;
                const size_t len = i % 5 == 0 ? 0 : i % 7 == 1 ? (size_t)l.run_len : unit * (size_t)(1 + i * 37 % 11) * 64;
                segs.push_back(RowSeg{(char *)((uintptr_t)0x100000000ull * (uintptr_t)(i + 1)), (char *)(0x10000000ull + (uintptr_t)i * 64), len});
            }
            check_plan(l, segs, 256, 2, 8, cap, true);
            std::vector<RowSeg> more(segs);
            more.push_back(segs[1]);
            ++checked;
            CHECK(plan_rows_multi(l.stride, l.extent, l.nblk, l.run_disp, l.run_len, more.data(), (int)more.size(), 512, 2048, cap).w == 0,
                  "more pieces than a launch holds were planned");
        }
    // the 32-bit limits: a piece of 2^36 bytes at W = 16 is one slot too many, just below is planned
    {
        const Layout l = layouts[1];
        std::vector<RowSeg> segs;
        segs.push_back(RowSeg{(char *)0x100000000ull, (char *)0x200000000ull, (size_t)kSlot32Max * 16});
        check_plan(l, segs, 256, 2, 8, 262144, false);
        segs[0].len -= 16;
        check_plan(l, segs, 256, 2, 8, 262144, false);
        segs.push_back(RowSeg{(char *)0x300000000ull, (char *)0x400000000ull, 4096});
        check_plan(l, segs, 256, 2, 8, 262144, false);
    }
    std::printf("{\"checked\": %ld, \"mismatches\": %ld}\n", checked, fails);
    return fails ? 1 : 0;
}
