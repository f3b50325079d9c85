/* Host-sanitizer check of the coll/libnbc schedule code (csrc/rt/coll_nbc.cpp and its part of
 * mi355x_sched_program): a stand-alone program against the AddressSanitizer + UBSan build of the
 * library (csrc/Makefile.san -> ompi-release_amd/lib_san).  It walks every program kind 6-8 for 1..64
 * ranks, every root and ring segment, and the partition and selection calls, and checks that each
 * program names every rank exactly once.  CPU only, no GPU is touched.
 *
 *   make -C ompi-release_amd/csrc -f Makefile.san -j8
 *   R=<the sanitizer runtime's directory: SANRT of csrc/Makefile.san>
 *   /opt/rocm/lib/llvm/bin/clang -O1 -g -fsanitize=address,undefined -shared-libsan -Iinclude \
 *       -o /tmp/nbc_san tools/nbc_san.c -Lompi-release_amd/lib_san -lmi355x_rt \
 *       -Wl,-rpath,$PWD/ompi-release_amd/lib_san -Wl,-rpath,$R
 *   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/nbc_san
 */
#include <stdio.h>
#include <string.h>

#include "mi355x_rt.h"

static int fails;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            fails++;                  \
            fprintf(stderr, __VA_ARGS__); \
            fputc('\n', stderr);      \
        }                             \
    } while (0)

/* every rank 0..n-1 is read exactly once by the program in v[0..k) */
static void every_rank_once(const int *v, int k, int n, const char *what)
{
    int seen[64];
    memset(seen, 0, sizeof(seen));
    CHECK(k >= 3 && (v[0] == 2 || v[0] == 3), "%s: layout %d", what, k > 0 ? v[0] : -1);
    if (k < 3) return;
    if (v[0] == 3) {
        CHECK(v[2] == n && k == 3 + 2 * n, "%s: fold over %d of %d ranks", what, v[2], n);
        for (int j = 0; j < v[2] && 3 + j < k; ++j) {
            const int r = v[3 + j];
            CHECK(r >= 0 && r < n && !seen[r]++, "%s: rank %d", what, r);
        }
        return;
    }
    CHECK(v[2] == n - 1 && k == 4 + 3 * v[2], "%s: %d steps for %d ranks", what, v[2], n);
    for (int s = 0; s < v[2] && 6 + 3 * s < k; ++s) {
        const int d = v[4 + 3 * s], o = v[5 + 3 * s], i = v[6 + 3 * s];
        CHECK(d == o && o >= 0 && o < n && i >= 0 && i < n && o != i, "%s: step (%d, %d, %d)", what, d, o, i);
        if (i >= 0 && i < n) CHECK(!seen[i]++, "%s: register %d consumed twice", what, i);
    }
    CHECK(v[3] >= 0 && v[3] < n && !seen[v[3]], "%s: result register %d", what, v[3]);
}

int main(void)
{
    static int v[4096];
    char what[96];
    for (int n = 1; n <= 64; ++n) {
        for (int b = 0; b < n; ++b) {
            const int kinds[5][2] = {{6, 101}, {6, 102}, {7, 101}, {7, 103}, {8, 0}};
            for (int c = 0; c < 5; ++c) {
                const int tree = kinds[c][1] != 102 && kinds[c][1] != 103;
                const int k = mi355x_sched_program(kinds[c][0], n, kinds[c][1], b, v, 4096);
                snprintf(what, sizeof(what), "kind %d alg %d n %d block %d", kinds[c][0], kinds[c][1], n, b);
                if (tree && n > 16) {
                    CHECK(k == MI355X_ERR_UNSUPPORTED, "%s: %d, not MI355X_ERR_UNSUPPORTED", what, k);
                    continue;
                }
                CHECK(k > 0, "%s: %d (%s)", what, k, mi355x_last_error());
                if (k > 0) every_rank_once(v, k, n, what);
            }
        }
        CHECK(mi355x_sched_program(6, n, 102, n, v, 4096) == MI355X_ERR_ARG, "segment %d of %d accepted", n, n);
        CHECK(mi355x_sched_program(7, n, 102, 0, v, 4096) == MI355X_ERR_ARG, "ireduce has no ring");
        CHECK(mi355x_sched_program(6, n, 101, 0, v, 2) < 0, "cap 2 accepted");
        const size_t counts[] = {0, 1, 10, 2049, 16385, (size_t)1 << 32, ~(size_t)0 >> 8};
        for (unsigned ci = 0; ci < sizeof(counts) / sizeof(counts[0]); ++ci) {
            size_t pos = 0, off, len;
            for (int e = 0; e < n; ++e) {
                CHECK(mi355x_nbc_ring_block(counts[ci], n, e, &off, &len) == MI355X_SUCCESS, "ring block");
                CHECK(off == pos, "count %zu n %d segment %d starts at %zu, not %zu", counts[ci], n, e, off, pos);
                pos += len;
            }
            CHECK(pos == counts[ci], "count %zu n %d: segments cover %zu", counts[ci], n, pos);
        }
        CHECK(mi355x_nbc_ring_block(10, n, n, &(size_t){0}, &(size_t){0}) == MI355X_ERR_ARG, "segment n accepted");
        for (int coll = 0; coll < 3; ++coll)
            for (int inplace = 0; inplace < 2; ++inplace) {
                const int a = mi355x_nbc_decision(coll, n, 65536, inplace), b = mi355x_nbc_decision(coll, n, 65535, inplace);
                CHECK(a >= 101 && a <= 103 && b == 101, "decision coll %d n %d: %d %d", coll, n, a, b);
            }
    }
    CHECK(mi355x_nbc_decision(4, 4, 1, 0) == MI355X_ERR_ARG && mi355x_nbc_decision(0, 65, 1, 0) == MI355X_ERR_ARG, "bad arguments accepted");
    printf(fails ? "nbc_san: %d FAILED\n" : "nbc_san: OK\n", fails);
    return fails ? 1 : 0;
}
