/* Host-sanitizer check of MPI_Ireduce_scatter's host code: mi355x_sched_program kind 9 and
 * mi355x_nbc_decision(3, ...) (csrc/rt/coll_nbc.cpp, coll_comm.cpp), and what mi355x_ireduce_scatter
 * (csrc/rt/coll_flows.cpp) decides in the posting call before any device work -- its argument checks,
 * the copy of the counts, the 16-rank limit of libnbc's order and the completed request of an empty
 * vector.  A stand-alone program against the AddressSanitizer + UBSan build of the library
 * (csrc/Makefile.san -> ompi-release_amd/lib_san).  CPU only, no GPU is touched.
 *
 *   make -C ompi-release_amd/csrc -f Makefile.san -j8
 *   R=<the sanitizer runtime's directory: SANRT of csrc/Makefile.san>
 *   /opt/rocm/lib/llvm/bin/clang -O1 -g -fsanitize=address,undefined -shared-libsan -Iinclude \
 *       -o /tmp/irs_san tools/irs_san.c -Lompi-release_amd/lib_san -lmi355x_rt \
 *       -Wl,-rpath,$PWD/ompi-release_amd/lib_san -Wl,-rpath,$R
 *   ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=halt_on_error=1 /tmp/irs_san
 */
#include <stdio.h>
#include <stdlib.h>
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

enum { T_FLOAT = MI355X_T_FLOAT, OP_SUM = MI355X_OP_SUM, OP_NULL = MI355X_OP_NULL };

int main(void)
{
    static int v9[4096], v8[4096];
    for (int n = 1; n <= 17; ++n) {
        for (int b = 0; b < n; ++b) {
            const int k9 = mi355x_sched_program(9, n, 101, b, v9, 4096), k8 = mi355x_sched_program(8, n, 0, b, v8, 4096);
            if (n > 16) {
                CHECK(k9 == MI355X_ERR_UNSUPPORTED, "kind 9 n %d block %d: %d, not MI355X_ERR_UNSUPPORTED", n, b, k9);
                continue;
            }
            CHECK(k9 > 0 && k9 == k8 && !memcmp(v9, v8, (size_t)k9 * sizeof(int)), "kind 9 n %d block %d: %d ints, kind 8 %d (%s)",
                  n, b, k9, k8, mi355x_last_error());
        }
        CHECK(mi355x_sched_program(9, n, 101, n, v9, 4096) == MI355X_ERR_ARG, "block %d of %d accepted", n, n);
        CHECK(mi355x_sched_program(9, n, 101, -1, v9, 4096) == MI355X_ERR_ARG, "block -1 accepted");
        CHECK(mi355x_sched_program(9, n, 101, 0, v9, 1) < 0, "cap 1 accepted");
        CHECK(mi355x_nbc_decision(3, n, 65535, 0) == 101 && mi355x_nbc_decision(3, n, 65536, 0) == 101 &&
              mi355x_nbc_decision(3, n, 0, 1) == 101, "decision coll 3 n %d", n);
    }
    CHECK(mi355x_nbc_decision(3, 0, 1, 0) == MI355X_ERR_ARG && mi355x_nbc_decision(3, 65, 1, 0) == MI355X_ERR_ARG &&
          mi355x_nbc_decision(4, 4, 1, 0) == MI355X_ERR_ARG, "bad arguments accepted");

    /* the posting call, on loopback communicators (host objects: nothing on the device is set up) */
    int counts[17];
    for (int i = 0; i < 17; ++i) counts[i] = 1;
    mi355x_request_t *req = NULL;
    char in[64], out[64];
    memset(out, 0x5a, sizeof(out));
    memset(in, 0, sizeof(in));
    CHECK(mi355x_ireduce_scatter(NULL, in, out, counts, T_FLOAT, OP_SUM, NULL, &req) == MI355X_ERR_ARG, "NULL communicator accepted");
    mi355x_comm_t *cs[17];
    for (int n = 3; n <= 17; n += 14) {
        CHECK(mi355x_comm_create_loopback(n, 0, cs) == MI355X_SUCCESS, "loopback %d: %s", n, mi355x_last_error());
        if (fails) break;
        for (int order = 0; order < 2; ++order) {
            for (int r = 0; r < n; ++r) CHECK(mi355x_comm_set(cs[r], MI355X_KNOB_NB_ORDER, order) == MI355X_SUCCESS, "nb_order");
            mi355x_comm_t *c = cs[n - 1];
            CHECK(mi355x_ireduce_scatter(c, in, out, NULL, T_FLOAT, OP_SUM, NULL, &req) == MI355X_ERR_ARG, "NULL rcounts accepted");
            CHECK(mi355x_ireduce_scatter(c, in, out, counts, T_FLOAT, OP_SUM, NULL, NULL) == MI355X_ERR_ARG, "NULL req accepted");
            CHECK(mi355x_ireduce_scatter(c, in, out, counts, T_FLOAT, OP_NULL, NULL, &req) != MI355X_SUCCESS, "MPI_OP_NULL accepted");
            CHECK(mi355x_ireduce_scatter(c, in, out, counts, -1, OP_SUM, NULL, &req) != MI355X_SUCCESS, "type -1 accepted");
            counts[n - 1] = -1;
            CHECK(mi355x_ireduce_scatter(c, in, out, counts, T_FLOAT, OP_SUM, NULL, &req) == MI355X_ERR_ARG, "negative count accepted");
            counts[n - 1] = 1;
            if (order == 1 && n > 16) {   /* libnbc's tree does not fit: every rank gets this answer, nothing is queued */
                for (int r = 0; r < n; ++r) {
                    req = NULL;
                    CHECK(mi355x_ireduce_scatter(cs[r], in, out, counts, T_FLOAT, OP_SUM, NULL, &req) == MI355X_ERR_UNSUPPORTED && !req,
                          "17 ranks in libnbc's order accepted on rank %d", r);
                }
                continue;
            }
            /* an empty vector: a completed request, no buffer touched; the counts live on the heap so
             * that a read after the call has returned would be caught */
            int *zero = calloc((size_t)n, sizeof(int));
            req = NULL;
            CHECK(mi355x_ireduce_scatter(c, in, out, zero, T_FLOAT, OP_SUM, NULL, &req) == MI355X_SUCCESS && req, "empty vector: %s",
                  mi355x_last_error());
            free(zero);
            if (req) {
                int done = 0;
                CHECK(mi355x_request_test(req, &done) == MI355X_SUCCESS && done == 1, "empty vector: request not complete");
                CHECK(mi355x_request_wait(req) == MI355X_SUCCESS && mi355x_request_free(req) == MI355X_SUCCESS, "empty vector: wait / free");
            }
            for (unsigned i = 0; i < sizeof(out); ++i) CHECK(out[i] == 0x5a, "empty vector: rbuf byte %u written", i);
            CHECK(mi355x_comm_set(c, MI355X_KNOB_NB_ORDER, order) == MI355X_SUCCESS, "nothing is pending after these calls");
        }
        for (int r = 0; r < n; ++r) mi355x_comm_destroy(cs[r]);
    }
    printf(fails ? "irs_san: %d FAILED\n" : "irs_san: OK\n", fails);
    return fails ? 1 : 0;
}
