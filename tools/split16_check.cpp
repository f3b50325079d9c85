// split16_check.cpp -- (check, host only) the head / 16-B body / tail split every bandwidth kernel
// takes from ompi-release_amd/csrc/rt/stream_core.hpp, against its definition written out by brute
// force: every n in 0..70, element size in {1, 2, 4, 8, 16}, misalignment m in 0..15 and both values
// of the co-aligned flag; and co_aligned over pointer lists at every pair of misalignments.
// Stand-alone, under the host sanitizers; prints one JSON line, exit status 1 on any mismatch.
//   make -C tools check
#define MI_HD inline
#include "../ompi-release_amd/csrc/rt/stream_core.hpp"

#include <cstdio>

using mi355x::Split16;

static long fails, checked;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            fails++;                      \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fputc('\n', stderr);     \
        }                                 \
    } while (0)

// the definition, element by element: walk scalar elements until the address is a multiple of 16
// (or the range ends), then count the whole vectors that still fit
static Split16 brute(size_t n, size_t esz, size_t m, bool co)
{
    if (!co || m % esz != 0) return Split16{n, 0};
    size_t head = 0;
    while (head < n && (m + head * esz) % 16 != 0) ++head;
    size_t nvec = 0;
    while ((head + (nvec + 1) * (16 / esz)) <= n) ++nvec;
    return Split16{head, nvec};
}

int main()
{
    static const size_t sizes[] = {1, 2, 4, 8, 16};
    for (size_t n = 0; n <= 70; ++n)
        for (size_t esz : sizes)
            for (size_t m = 0; m < 16; ++m)
                for (int co = 0; co < 2; ++co) {
                    const Split16 s = mi355x::split16(n, esz, m, co != 0);
                    const Split16 w = brute(n, esz, m, co != 0);
                    const size_t epv = 16 / esz;
                    ++checked;
                    CHECK(s.head == w.head && s.nvec == w.nvec, "n %zu esz %zu m %zu co %d: head %zu nvec %zu, want %zu %zu",
                          n, esz, m, co, s.head, s.nvec, w.head, w.nvec);
                    if (!co || m % esz != 0) {
                        CHECK(s.head == n && s.nvec == 0, "n %zu esz %zu m %zu co %d: not element-wise", n, esz, m, co);
                    } else {
                        const size_t h = m ? (16 - m) / esz : 0;
                        CHECK(s.head == (h < n ? h : n), "n %zu esz %zu m %zu: head %zu", n, esz, m, s.head);
                    }
                    CHECK(s.nvec == (n - s.head) / epv, "n %zu esz %zu m %zu co %d: nvec %zu", n, esz, m, co, s.nvec);
                    CHECK(s.nvec == 0 || (m + s.head * esz) % 16 == 0, "n %zu esz %zu m %zu: body not 16-B aligned", n, esz, m);
                    CHECK(s.head + s.nvec * epv <= n, "n %zu esz %zu m %zu co %d: split exceeds the range", n, esz, m, co);
                }
    // co_aligned: m comes from the first pointer, must be a whole element, and every pointer shares it
    alignas(16) static char buf[3][64];
    for (size_t esz : sizes)
        for (size_t m0 = 0; m0 < 16; ++m0)
            for (size_t m1 = 0; m1 < 16; ++m1)
                for (int np = 1; np <= 3; ++np) {
                    const void *p[3] = {buf[0] + m0, buf[1] + m0, buf[2] + m1};
                    const bool want = m0 % esz == 0 && (np < 3 || m1 == m0);
                    ++checked;
                    CHECK(mi355x::co_aligned(esz, p, np) == want, "co_aligned esz %zu m0 %zu m1 %zu np %d", esz, m0, m1, np);
                }
    std::printf("{\"checked\": %ld, \"mismatches\": %ld}\n", checked, fails);
    return fails ? 1 : 0;
}
