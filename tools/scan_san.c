/* Host-sanitizer check of the partitioned scan flow's host code (csrc/rt/coll_move.cpp:
 * mi355x_scan_part_plan, the layout the flow and the tests share) and of the knob that selects the
 * flow: a stand-alone program against the AddressSanitizer + UBSan build of the library
 * (csrc/Makefile.san -> ompi-release_amd/lib_san).  It walks the plan for 1..64 ranks, every owner
 * and every destination, at counts from 0 to beyond 2^32 elements, and checks that the blocks tile
 * the vector, that an owner's slots are disjoint and stay inside the scratch the flow allocates
 * ((n - 1) slots of the block's length), and that bad arguments and knob values are rejected.
 * CPU only, no GPU is touched.
 *
 *   make -C ompi-release_amd/csrc -f Makefile.san -j8
 *   R=<the sanitizer runtime's directory: SANRT of csrc/Makefile.san>
 *   /opt/rocm/lib/llvm/bin/clang -O1 -g -fsanitize=address,undefined -shared-libsan -Iinclude \
 *       -o /tmp/scan_san tools/scan_san.c -Lompi-release_amd/lib_san -lmi355x_rt \
 *       -Wl,-rpath,$PWD/ompi-release_amd/lib_san -Wl,-rpath,$R
 *   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/scan_san
 */
#include <stdint.h>
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

int main(void)
{
    for (int n = 1; n <= 64; ++n) {
        const size_t counts[] = {0, 1, (size_t)n - 1, (size_t)n, 1000 * (size_t)n + 7, 16385, (size_t)1 << 32,
                                 ~(size_t)0 >> 8};
        for (unsigned ci = 0; ci < sizeof(counts) / sizeof(counts[0]); ++ci) {
            const size_t count = counts[ci];
            size_t pos = 0;
            for (int q = 0; q < n; ++q) {
                size_t off = 0, len = 0, slot = 0;
                CHECK(mi355x_scan_part_plan(count, n, q, q, &off, &len, &slot) == MI355X_SUCCESS, "plan n %d q %d", n, q);
                CHECK(slot == SIZE_MAX, "n %d owner %d: its own prefix has scratch slot %zu", n, q, slot);
                CHECK(off == pos, "count %zu n %d block %d starts at %zu, not %zu", count, n, q, off, pos);
                pos += len;
                unsigned char used[64];
                memset(used, 0, sizeof(used));
                for (int r = 0; r < n; ++r) {
                    size_t o2 = 0, l2 = 0, s2 = 0;
                    if (r == q) continue;
                    CHECK(mi355x_scan_part_plan(count, n, q, r, &o2, &l2, &s2) == MI355X_SUCCESS, "plan n %d q %d r %d", n, q, r);
                    CHECK(o2 == off && l2 == len, "n %d q %d r %d: another block", n, q, r);
                    if (len == 0) continue;
                    const size_t idx = s2 / len;   /* slots are whole multiples of the block's length */
                    CHECK(s2 % len == 0 && idx < (size_t)(n - 1), "n %d q %d r %d: slot %zu of %zu-element slots", n, q, r, s2, len);
                    if (idx < 64) CHECK(!used[idx]++, "n %d q %d: slot %zu given twice", n, q, idx);
                }
            }
            CHECK(pos == count, "count %zu n %d: blocks cover %zu", count, n, pos);
        }
        size_t a, b, c;
        CHECK(mi355x_scan_part_plan(10, n, n, 0, &a, &b, &c) == MI355X_ERR_ARG, "owner n accepted");
        CHECK(mi355x_scan_part_plan(10, n, 0, -1, &a, &b, &c) == MI355X_ERR_ARG, "rank -1 accepted");
        CHECK(mi355x_scan_part_plan(10, n, 0, 0, NULL, &b, &c) == MI355X_ERR_ARG, "NULL output accepted");
    }
    size_t a, b, c;
    CHECK(mi355x_scan_part_plan(10, 0, 0, 0, &a, &b, &c) == MI355X_ERR_ARG &&
          mi355x_scan_part_plan(10, 65, 0, 0, &a, &b, &c) == MI355X_ERR_ARG, "bad communicator size accepted");
    /* the knob, on loopback communicators (host objects: nothing on the device is set up) */
    mi355x_comm_t *cs[3];
    CHECK(mi355x_comm_create_loopback(3, 0, cs) == MI355X_SUCCESS, "loopback: %s", mi355x_last_error());
    if (!fails) {
        const long vals[] = {0, 1, 65536, 1l << 40};
        for (int r = 0; r < 3; ++r)
            for (unsigned i = 0; i < sizeof(vals) / sizeof(vals[0]); ++i) {
                long got = -1;
                CHECK(mi355x_comm_set(cs[r], MI355X_KNOB_SCAN_PART_MIN_BYTES, vals[i]) == MI355X_SUCCESS, "set %ld", vals[i]);
                CHECK(mi355x_comm_get(cs[r], MI355X_KNOB_SCAN_PART_MIN_BYTES, &got) == MI355X_SUCCESS && got == vals[i],
                      "get %ld after set %ld", got, vals[i]);
            }
        CHECK(mi355x_comm_set(cs[0], MI355X_KNOB_SCAN_PART_MIN_BYTES, -1) == MI355X_ERR_ARG, "-1 accepted");
        for (int r = 0; r < 3; ++r) mi355x_comm_destroy(cs[r]);
    }
    printf(fails ? "scan_san: %d FAILED\n" : "scan_san: OK\n", fails);
    return fails ? 1 : 0;
}
