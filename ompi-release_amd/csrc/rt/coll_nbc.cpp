// coll_nbc.cpp -- coll/libnbc's operand order for the nonblocking reductions.
//
// In the reference MPI_Iallreduce, MPI_Ireduce and MPI_Ireduce_scatter(_block) belong to coll/libnbc
// (coll/cuda fills no nonblocking slot): libnbc picks its own algorithms with its own thresholds
// and applies every reduction step as a 3-buff call, target = in1 (op) in2, with the rank's own
// data as in1 (NBC_Sched_op, nbc.c:123-145; ompi_3buff_op_reduce, nbc.c:446-467).  This file
// restates those schedules symbolically, as coll_sched.cpp restates coll/tuned's, and holds the
// MPI_Iallreduce flow that evaluates them.  A communicator runs them when MI355X_KNOB_NB_ORDER is 1;
// the default (0) keeps coll/tuned's order for the nonblocking calls, as for the blocking ones.
//
// Flows that serve a libnbc-ordered call: the one-launch evaluation from the mapped inputs (k_fold,
// k_tree, k_ring_all's libnbc form), owner-computes + pull, the staged flow and gather-then-fold.
// The LL, resident-service and pipelined kernels apply the 2-buff rule and fix coll/tuned's ring
// order inside the kernel: such a call never takes them.
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "coll_internal.hpp"
#include "coll_sched.hpp"
#include "rt_internal.hpp"

#include "comm_internal.hpp"

#include "coll_comm_int.hpp"

namespace mi355x {

// ----------------------------------------------------------------- decisions
int nbc_iallreduce_decision(int n, size_t count, size_t dsize, bool inplace)
{
    return (n < 4 || dsize * count < 65536 || inplace) ? NBC_BINOMIAL : NBC_RING;
}

int nbc_ireduce_decision(int n, size_t count, size_t dsize)
{
    return (n > 4 || dsize * count < 65536) ? NBC_BINOMIAL : NBC_CHAIN;
}

// ----------------------------------------------------------------- expressions
// RANK2VRANK / VRANK2RANK (nbc_ireduce.c:211-222): rank 0 and the root trade places (an involution)
static int vswap(int v, int root) { return v == 0 ? root : (v == root ? 0 : v); }

int expr_nbc_binomial(ExprPool &p, int n, int root)
{
    // round r = 1, 2, ...: a virtual rank that is a multiple of 2^r receives from vrank + 2^(r-1)
    // (if that rank exists) and reduces -- the first time own (op) received, from then on
    // running (op) received -- any other sends what it has and leaves (nbc_ireduce.c:229-282)
    std::function<int(int)> value = [&](int v) -> int {
        int acc = p.leaf(vswap(v, root));
        for (int r = 1; (v % (1 << r)) == 0 && (1 << (r - 1)) < n; ++r) {
            const int vpeer = v + (1 << (r - 1));
            if (vpeer < n) acc = p.op(acc, value(vpeer));
        }
        return acc;
    };
    return value(0);
}

int expr_nbc_reduce_chain(ExprPool &p, int n, int root)
{
    // virtual rank v receives from v + 1 and computes own (op) received; v = n - 1 sends its own
    // data (nbc_ireduce.c:311-336).  The fragments cover disjoint elements: no element's order changes.
    int acc = p.leaf(vswap(n - 1, root));
    for (int v = n - 2; v >= 0; --v) acc = p.op(p.leaf(vswap(v, root)), acc);
    return acc;
}

Program nbc_ring_segment_program(int n, int e)
{
    // round 0: rank e - 1 sends its segment e to rank e, which computes own (op) received; each
    // later round passes the partial one rank on (nbc_iallreduce.c:436-455), n - 1 reductions
    Program pr;
    pr.is_fold = true;
    pr.nr = n;
    for (int j = 0; j < n; ++j) pr.order.push_back((e + n - 1 + j) % n);
    pr.role_mask = 0;  // the accumulator is in2 at every step
    pr.three = true;
    return pr;
}

void nbc_ring_block(size_t count, int n, int e, size_t *off, size_t *len)
{
    const size_t seg = (count + (size_t)n - 1) / (size_t)n;
    const size_t lo = std::min(count, (size_t)e * seg);
    *off = lo;
    *len = std::min(seg, count - lo);
}

bool nbc_program(int coll, int n, int alg, int block, Program *out)
{
    if (coll == 0 && alg == NBC_RING) {
        *out = nbc_ring_segment_program(n, block);
        return true;
    }
    ExprPool ep;
    int root;
    if (coll == 1 && alg == NBC_CHAIN) root = expr_nbc_reduce_chain(ep, n, block);
    else if (alg == NBC_BINOMIAL) root = expr_nbc_binomial(ep, n, coll == 1 ? block : 0);
    else return false;
    if (!compile_expr(ep, root, n, out)) return false;
    out->three = true;
    return true;
}

bool nbc_reduce_program(const mi355x_comm *c, size_t count, size_t esz, int root, Program *pr, int *alg)
{
    *alg = root < 0 ? (int)NBC_BINOMIAL : nbc_ireduce_decision(c->size, count, esz);
    return nbc_program(root < 0 ? 2 : 1, c->size, *alg, root < 0 ? 0 : root, pr);
}

int nbc_check(const mi355x_comm *c, int coll, size_t count, int type, bool inplace, int root)
{
    const size_t esz = mi355x_type_size(type);
    Program pr;
    bool ok;
    if (coll == 0) {
        const int alg = nbc_iallreduce_decision(c->size, count, esz, inplace);
        ok = alg == NBC_RING || nbc_program(0, c->size, alg, 0, &pr);
    } else {
        int alg;
        ok = nbc_reduce_program(c, count, esz, coll == 1 ? root : -1, &pr, &alg);
    }
    if (!ok)
        return set_error(MI355X_ERR_UNSUPPORTED, "coll/libnbc's binomial tree over %d ranks does not fit the device (%d)",
                         c->size, kTreeMax);
    return MI355X_SUCCESS;
}

// ----------------------------------------------------------------- MPI_Iallreduce
// libnbc's selection (binomial: every element one tree; ring: segment e its own fold), evaluated
//   one launch : (not in place, <= one_phase_max) every rank evaluates the whole vector from the n
//                mapped inputs into its own rbuf;
//   otherwise  : owner-computes -- rank r evaluates part r (the ring's segment r; for the binomial
//                any partition serves, coll/tuned's block r) into its rbuf, then pulls the others;
//   staged     : the same parts through the staging buffers.
int nbc_allreduce_impl(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, void *stream)
{
    int rc = check_common(c, op, type);
    if (rc) return rc;
    if (count == 0) return MI355X_SUCCESS;
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    if (const int rs_ = dev_setup(c)) return rs_;
    const void *in = sbuf ? sbuf : rbuf;
    const bool inplace = (in == (const void *)rbuf);
    if (!coll_slot_supported(op, type)) return gfold_allreduce(c, in, rbuf, count, type, op, s, true);
    const size_t esz = mi355x_type_size(type);
    const int n = c->size, me = c->rank;
    const int alg = nbc_iallreduce_decision(n, count, esz, inplace);
    c->last_alg = alg;
    if (n == 1) {
        if (!inplace) MI_HIP(hipMemcpyAsync(rbuf, sbuf, count * esz, hipMemcpyDeviceToDevice, s));
        MI_HIP(hipStreamSynchronize(s));
        return MI355X_SUCCESS;
    }
    const bool ring = alg == NBC_RING;
    auto part = [&](int q, size_t *o, size_t *l) {
        if (ring) nbc_ring_block(count, n, q, o, l);
        else ring_block(count, n, q, o, l);
    };
    Program pr;
    if (!nbc_program(0, n, alg, me, &pr)) return set_error(MI355X_ERR_UNSUPPORTED, "schedule too large");
    MI_HIP(hipStreamSynchronize(s));  // every rank's input is complete before it is published
    const void *mine[2] = {in, rbuf};
    const uint64_t sig[4] = {101, count, (uint64_t)type, ((uint64_t)op << 1) | (inplace ? 1u : 0u)};
    std::vector<std::vector<void *>> P;
    bool staged = false;
    rc = exchange(c, 2, mine, sig, P, &staged);
    if (rc) return rc;
    size_t off, len;
    part(me, &off, &len);
    if (staged) {
        std::vector<size_t> boff(n), blen(n);
        for (int q = 0; q < n; ++q) part(q, &boff[q], &blen[q]);
        return staged_reduce(c, op, type, pr, in, boff, blen, (char *)rbuf + off * esz, true, rbuf, s);
    }
    if (!inplace && count * esz <= c->one_phase_max && count <= 0xffffffffull) {
        if (ring) {
            RingAllArgs ra;
            std::memset(&ra, 0, sizeof(ra));
            for (int q = 0; q < n; ++q) ra.src[q] = P[0][q];
            ra.dst = rbuf;
            ra.n = n;
            ra.count = (uint32_t)count;
            ra.seg = (uint32_t)((count + (size_t)n - 1) / (size_t)n);
            rc = launch_ring_all_slot(op, type, ra, s);
        } else {
            std::vector<void *> dst(1, rbuf);
            rc = run_program(op, type, pr, P[0], dst, 0, count, s);
        }
        if (rc) return rc;
        return finish(c, s);
    }
    // phase 1: my part, read from the n inputs, written into my rbuf (in place: every lane reads
    // its element of every input before it writes it, and no peer reads my part of my buffer);
    // phase 2: the other parts from their owners
    std::vector<void *> dst(1, rbuf);
    rc = run_program(op, type, pr, P[0], dst, off, len, s);
    if (rc) return rc;
    rc = finish(c, s);
    if (rc) return rc;
    MultiCopyArgs m;
    std::memset(&m, 0, sizeof(m));
    for (int q = 0; q < n; ++q) {
        size_t qo, ql;
        part(q, &qo, &ql);
        if (q == me || ql == 0) continue;
        m.src[m.nseg] = (const char *)P[1][q] + qo * esz;
        m.dst[m.nseg] = (char *)rbuf + qo * esz;
        m.len[m.nseg] = ql * esz;
        m.nseg++;
    }
    rc = launch_multicopy(m, s);
    if (rc) return rc;
    return finish(c, s);
}

} // namespace mi355x

using namespace mi355x;

extern "C" {

// host-only introspection (tests; no GPU): libnbc's selection for coll 0 = MPI_Iallreduce,
// 1 = MPI_Ireduce, 2 = MPI_Ireduce_scatter_block, 3 = MPI_Ireduce_scatter of `bytes` bytes over n ranks
int mi355x_nbc_decision(int coll, int n, size_t bytes, int inplace)
{
    if (n < 1 || n > kMaxRanks) return set_error(MI355X_ERR_ARG, "bad communicator size");
    switch (coll) {
    case 0: return nbc_iallreduce_decision(n, bytes, 1, inplace != 0);
    case 1: return nbc_ireduce_decision(n, bytes, 1);
    case 2:
    case 3: return NBC_BINOMIAL;  // (nbc_ireduce_scatter.c:37-164 has one schedule)
    default: return set_error(MI355X_ERR_ARG, "unknown collective %d", coll);
    }
}

int mi355x_nbc_ring_block(size_t count, int n, int e, size_t *off, size_t *len)
{
    if (!off || !len || n < 1 || n > kMaxRanks || e < 0 || e >= n) return set_error(MI355X_ERR_ARG, "bad arguments");
    nbc_ring_block(count, n, e, off, len);
    return MI355X_SUCCESS;
}

} // extern "C"
