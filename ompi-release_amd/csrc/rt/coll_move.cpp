// coll_move.cpp -- the remaining collectives of the reduction path's callers on device buffers:
// MPI_Gather(v), MPI_Scatter(v), MPI_Allgatherv, MPI_Alltoall(v) (data movement) and MPI_Scan /
// MPI_Exscan (reductions).  Without them the reference stages every such call through host memory
// (coll/cuda covers only the reductions, coll_cuda_module.c:118-140; everything else goes to
// tuned/basic over the PML, whose device path is ob1 RGET over smcuda).
//
// One data flow for all of them, MI355X-first: every rank publishes its send buffer (the IPC /
// dmabuf registration cache of coll_comm.cpp), meets the others, and PULLS what it must receive
// straight from the owners' memory with one k_multicopy launch (one segment per peer, so every
// xGMI link runs at once), then meets them again so no buffer is reused while a peer still reads
// it.  Counts and displacements a receiver cannot know (scatterv's at the root, alltoallv's
// senders') are published in the control segment next to the buffers.
//
// Scan / Exscan replicate coll/basic's linear chain (coll_basic_scan.c:40-120,
// coll_basic_exscan.c:40-110): rank r's result is ((x0 op x1) op ...) op x_r, each step
// ompi_op_reduce(op, partial, x_k) -- the partial is the `in` operand -- so rank r evaluates that
// left fold over the n inputs directly (k_fold, order 0..r, every step role `in`), bit-identical
// to the chain without its n-1 sequential hops.  Large messages are partitioned instead
// (scan_part): rank q evaluates ring block q of every rank's prefix in one pass (k_scan_part).
#include <cstring>

#include "comm_internal.hpp"
#include "coll_comm_int.hpp"
#include "ddt_internal.hpp"

namespace mi355x {

// The pull.  Plain bytes: k_multicopy.  With a receive layout (the _ddt forms) the segments' bytes
// are packed streams of `rddt`, each unpacked from where it lies -- the owner's memory -- into the
// layout at its destination (ddt_unpack_segments): no dense receive view, no second pass.
static int copy_segments(mi355x_comm *c, MultiCopyArgs &m, hipStream_t s, const mi355x_ddt *rddt = nullptr)
{
    if (m.nseg == 0) return MI355X_SUCCESS;
    if (!rddt) return launch_multicopy(m, s);
    c->move_fused++;
    return ddt_unpack_segments(rddt, m.src, m.dst, m.len, m.nseg, s);
}

// The receive side of a _ddt form as the impls take it.  A layout with gaps stays (d); a NULL one,
// or one whose instances leave no gap (ddt_contiguous for the largest count), becomes the plain
// form's byte counts and displacements, so such a call IS the plain call.
struct RecvSide {
    const mi355x_ddt *d;
    const size_t *counts, *displs;
    int64_t first = 0;  // a gap-free layout's first byte, from the piece's base (in displs already)
    std::vector<size_t> bytes;
    RecvSide(const mi355x_ddt *rddt, int n, const size_t *cnt, const size_t *dsp) : d(rddt), counts(cnt), displs(dsp)
    {
        if (!rddt || !cnt) return;
        size_t most = 0;
        for (int q = 0; q < n; ++q) most = std::max(most, cnt[q]);
        if (!ddt_contiguous(rddt, most, &first)) {
            first = 0;
            return;
        }
        const size_t sz = mi355x_ddt_size(rddt);
        bytes.resize(2 * (size_t)n);
        for (int q = 0; q < n; ++q) {
            bytes[(size_t)q] = cnt[q] * sz;
            bytes[(size_t)(n + q)] = (dsp ? dsp[q] : 0) + (size_t)first;
        }
        counts = bytes.data();
        if (dsp) displs = bytes.data() + n;
        d = nullptr;
    }
};

// bytes piece q of a receive side holds: rcounts are bytes, or with a layout instances of it
static size_t piece_bytes(const mi355x_ddt *rddt, size_t count)
{
    return rddt ? count * mi355x_ddt_size(rddt) : count;
}

static void add_seg(MultiCopyArgs &m, const void *src, void *dst, size_t len)
{
    if (len == 0 || src == dst) return;
    m.src[m.nseg] = src;
    m.dst[m.nseg] = dst;
    m.len[m.nseg] = len;
    m.nseg++;
}

static int check_comm(mi355x_comm *c, int root)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    if (c->size > kMaxSegs) return set_error(MI355X_ERR_UNSUPPORTED, "communicator larger than %d ranks", kMaxSegs);
    if (root < 0 || root >= c->size) return set_error(MI355X_ERR_ARG, "bad root %d", root);
    return MI355X_SUCCESS;
}

// MPI_Gatherv: the root pulls rank q's sbytes into rbuf + displs[q] (at most rcounts[q] bytes).
// sbuf NULL at the root = MPI_IN_PLACE (its block is already in rbuf).
// rddt (every impl below): NULL, or the receive layout -- rcounts are then instances of it, displs
// still bytes, and the pull unpacks (copy_segments); everything up to the launch is the plain form's,
// so a rank may call this form while its peers call the plain one.
static int gatherv_impl(mi355x_comm *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                        const size_t *displs, int root, void *stream, const mi355x_ddt *rddt = nullptr)
{
    int rc = check_comm(c, root);
    if (rc) return rc;
    const bool am_root = c->rank == root;
    if (!am_root) rddt = nullptr;  // (no receive side)
    if (rddt && !sbuf) return set_error(MI355X_ERR_UNSUPPORTED, "gatherv: MPI_IN_PLACE with a receive layout");
    if (am_root && (!rcounts || !displs)) return set_error(MI355X_ERR_ARG, "gatherv: counts at the root are NULL");
    if (!am_root && !sbuf && sbytes) return set_error(MI355X_ERR_ARG, "MPI_IN_PLACE is only valid at the root");
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    MI_HIP(hipStreamSynchronize(s));
    c->ctrl->slot[c->rank].varg[0] = (int64_t)(sbuf ? sbytes : 0);
    const void *mine[1] = {sbytes ? sbuf : nullptr};
    const uint64_t sig[4] = {20, (uint64_t)root, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    if (am_root) {
        MultiCopyArgs m;
        std::memset(&m, 0, sizeof(m));
        for (int q = 0; q < c->size; ++q) {
            const size_t qb = (size_t)c->ctrl->slot[q].varg[0];
            if (qb > piece_bytes(rddt, rcounts[q]))
                return set_error(MI355X_ERR_TRUNCATE, "gatherv: rank %d sends %zu bytes, root expects %zu", q, qb,
                                 piece_bytes(rddt, rcounts[q]));
            if (qb) add_seg(m, P[0][q], (char *)rbuf + displs[q], qb);
        }
        rc = copy_segments(c, m, s, rddt);
        if (rc) return rc;
    }
    return finish(c, s);
}

// MPI_Scatterv: rank r pulls scounts[r] bytes at root's sbuf + displs[r] (both published by the
// root) into rbuf (at most rbytes).  rbuf NULL at the root = MPI_IN_PLACE.
static int scatterv_impl(mi355x_comm *c, const void *sbuf, const size_t *scounts, const size_t *displs, void *rbuf,
                         size_t rbytes, int root, void *stream, const mi355x_ddt *rddt = nullptr)
{
    int rc = check_comm(c, root);
    if (rc) return rc;
    const bool am_root = c->rank == root;
    if (am_root && (!scounts || !displs)) return set_error(MI355X_ERR_ARG, "scatterv: counts at the root are NULL");
    if (!am_root && !rbuf && rbytes) return set_error(MI355X_ERR_ARG, "MPI_IN_PLACE is only valid at the root");
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    MI_HIP(hipStreamSynchronize(s));
    bool any = false;
    if (am_root)
        for (int q = 0; q < c->size; ++q) {
            c->ctrl->slot[c->rank].varg[q] = (int64_t)scounts[q];
            c->ctrl->slot[c->rank].varg[kMaxRanks + q] = (int64_t)displs[q];
            any = any || scounts[q];
        }
    const void *mine[1] = {am_root && any ? sbuf : nullptr};
    const uint64_t sig[4] = {21, (uint64_t)root, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    const RankSlot &rs = c->ctrl->slot[root];
    const size_t len = (size_t)rs.varg[c->rank];
    if (rbuf && len) {
        if (len > piece_bytes(rddt, rbytes))
            return set_error(MI355X_ERR_TRUNCATE, "scatterv: root sends %zu bytes to rank %d, which expects %zu", len,
                             c->rank, piece_bytes(rddt, rbytes));
        MultiCopyArgs m;
        std::memset(&m, 0, sizeof(m));
        add_seg(m, (const char *)P[0][root] + rs.varg[kMaxRanks + c->rank], rbuf, len);
        rc = copy_segments(c, m, s, rddt);
        if (rc) return rc;
    }
    return finish(c, s);
}

// MPI_Allgatherv: every rank pulls rank q's block (rcounts[q] bytes) into rbuf + displs[q].
// sbuf NULL = MPI_IN_PLACE (the rank's block is at rbuf + displs[rank]).
static int allgatherv_impl(mi355x_comm *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                           const size_t *displs, void *stream, const mi355x_ddt *rddt = nullptr)
{
    int rc = check_comm(c, 0);
    if (rc) return rc;
    if (!rcounts || !displs) return set_error(MI355X_ERR_ARG, "allgatherv: counts are NULL");
    if (rddt && !sbuf) return set_error(MI355X_ERR_UNSUPPORTED, "allgatherv: MPI_IN_PLACE with a receive layout");
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    MI_HIP(hipStreamSynchronize(s));
    const int me = c->rank;
    const void *src = sbuf ? sbuf : (const char *)rbuf + displs[me];
    const size_t mybytes = sbuf ? sbytes : rcounts[me];
    if (mybytes > piece_bytes(rddt, rcounts[me]))
        return set_error(MI355X_ERR_TRUNCATE, "allgatherv: rank %d sends %zu bytes, %zu expected", me, mybytes,
                         piece_bytes(rddt, rcounts[me]));
    const void *mine[1] = {mybytes ? src : nullptr};
    const uint64_t sig[4] = {22, 0, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    MultiCopyArgs m;
    std::memset(&m, 0, sizeof(m));
    for (int q = 0; q < c->size; ++q)
        if (rcounts[q] && P[0][q])
            add_seg(m, P[0][q], (char *)rbuf + displs[q], q == me ? mybytes : piece_bytes(rddt, rcounts[q]));
    rc = copy_segments(c, m, s, rddt);
    if (rc) return rc;
    return finish(c, s);
}

// MPI_Alltoallv: rank r pulls from rank q the scounts_q[r] bytes at q's sbuf + sdispls_q[r]
// (published by q) into rbuf + rdispls[q] (at most rcounts[q]).  sbuf NULL = MPI_IN_PLACE: the
// data to send is rbuf laid out by rcounts / rdispls, snapshotted into scratch first.
static int alltoallv_impl(mi355x_comm *c, const void *sbuf, const size_t *scounts, const size_t *sdispls, void *rbuf,
                          const size_t *rcounts, const size_t *rdispls, void *stream, const mi355x_ddt *rddt = nullptr)
{
    int rc = check_comm(c, 0);
    if (rc) return rc;
    if (!rcounts || !rdispls || (sbuf && (!scounts || !sdispls)))
        return set_error(MI355X_ERR_ARG, "alltoallv: counts are NULL");
    if (rddt && !sbuf) return set_error(MI355X_ERR_UNSUPPORTED, "alltoallv: MPI_IN_PLACE with a receive layout");
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    const int n = c->size, me = c->rank;
    const void *src = sbuf;
    if (!sbuf) {
        scounts = rcounts;
        sdispls = rdispls;
        size_t extent = 0;
        for (int q = 0; q < n; ++q) extent = std::max(extent, rdispls[q] + rcounts[q]);
        if (extent) {
            rc = ensure_scratch(c, extent);
            if (rc) return rc;
            MI_HIP(hipMemcpyAsync(c->scratch, rbuf, extent, hipMemcpyDeviceToDevice, s));
        }
        src = c->scratch;
    }
    MI_HIP(hipStreamSynchronize(s));
    bool any = false;
    for (int q = 0; q < n; ++q) {
        c->ctrl->slot[me].varg[q] = (int64_t)scounts[q];
        c->ctrl->slot[me].varg[kMaxRanks + q] = (int64_t)sdispls[q];
        any = any || scounts[q];
    }
    const void *mine[1] = {any ? src : nullptr};
    const uint64_t sig[4] = {23, 0, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    MultiCopyArgs m;
    std::memset(&m, 0, sizeof(m));
    for (int k = 0; k < n; ++k) {
        const int q = (me + k) % n;   // own block first, then the peers in ring order
        const RankSlot &qs = c->ctrl->slot[q];
        const size_t len = (size_t)qs.varg[me];
        if (len > piece_bytes(rddt, rcounts[q]))
            return set_error(MI355X_ERR_TRUNCATE, "alltoallv: rank %d sends %zu bytes to rank %d, which expects %zu",
                             q, len, me, piece_bytes(rddt, rcounts[q]));
        if (len) add_seg(m, (const char *)P[0][q] + qs.varg[kMaxRanks + me], (char *)rbuf + rdispls[q], len);
    }
    rc = copy_segments(c, m, s, rddt);
    if (rc) return rc;
    return finish(c, s);
}

// The partitioned flow's layout (host only; shared with the tests): owner q evaluates ring block q
// = elements [src_off, src_off + len) of every prefix.  Rank q's own prefix goes straight into its
// rbuf (slot_off = SIZE_MAX for r == q); rank r's sits in q's scratch at element slot_off: n - 1
// slots of len elements, rank r's at index r (r < q) or r - 1 (r > q).
static void scan_part_plan(size_t count, int n, int q, int r, size_t *src_off, size_t *len, size_t *slot_off)
{
    ring_block(count, n, q, src_off, len);
    *slot_off = r == q ? SIZE_MAX : (size_t)(r < q ? r : r - 1) * *len;
}

// MPI_Scan / MPI_Exscan, owner-computes: rank q evaluates block q of EVERY
// rank's prefix in one k_scan_part launch over the mapped inputs -- its own prefix into its rbuf,
// the others' into its scratch (local writes only) -- and after the meeting point every rank pulls
// its n - 1 other blocks out of the owners' scratch (k_multicopy, one segment per owner).  Each
// input element is read once across the communicator instead of up to n times by the last rank,
// and the bits are the chain's: a prefix is a chain, so the running accumulator of element i is
// rank k's result after step k.  In place needs no extra copy: owner q is the only reader of
// block q of anybody's input, and it is done before the meeting point that precedes the pulls.
// *staged: a buffer cannot be exported -- nothing was done, the caller takes the chain flow.
static int scan_part(mi355x_comm *c, const void *in, void *rbuf, size_t count, int type, int op, bool exclusive,
                     bool three, hipStream_t s, bool *staged)
{
    const size_t esz = mi355x_type_size(type);
    const int n = c->size, me = c->rank;
    size_t off, len, so;
    scan_part_plan(count, n, me, me, &off, &len, &so);
    int rc;
    if (len) {
        rc = ensure_scratch(c, (size_t)(n - 1) * len * esz);
        if (rc) return rc;
    }
    MI_HIP(hipStreamSynchronize(s));
    const void *mine[2] = {in, len ? c->scratch : nullptr};
    const uint64_t sig[4] = {exclusive ? 27u : 26u, count, ((uint64_t)type << 32) | (uint64_t)op, three ? 1u : 0u};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 2, mine, sig, P, staged);
    if (rc || *staged) return rc;
    c->last_alg = 2;
    if (len) {  // phase 1: block `me` of every prefix
        ScanArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nr = n;
        a.exclusive = exclusive ? 1 : 0;
        a.three = three ? 1 : 0;
        a.n = len;
        for (int k = 0; k < n; ++k) {
            size_t o, l, slot;
            scan_part_plan(count, n, me, k, &o, &l, &slot);
            a.src[k] = (const char *)P[0][k] + off * esz;
            a.dst[k] = k == me ? (char *)rbuf + off * esz : (char *)c->scratch + slot * esz;
        }
        rc = launch_scan_slot(op, type, a, s);
        if (rc) return rc;
    }
    rc = finish(c, s);  // every owner is done with every input and has its prefixes in place
    if (rc) return rc;
    if (!(exclusive && me == 0)) {  // phase 2: my prefix's other blocks, from their owners
        MultiCopyArgs m;
        std::memset(&m, 0, sizeof(m));
        for (int k = 1; k < n; ++k) {
            const int q = (me + k) % n;
            size_t qo, ql, slot;
            scan_part_plan(count, n, q, me, &qo, &ql, &slot);
            if (ql == 0) continue;
            if (m.nseg == kMaxSegs) {  // (more owners than one launch holds: split the pull)
                rc = copy_segments(c, m, s);
                if (rc) return rc;
                std::memset(&m, 0, sizeof(m));
            }
            add_seg(m, (const char *)P[1][q] + slot * esz, (char *)rbuf + qo * esz, ql * esz);
        }
        rc = copy_segments(c, m, s);
        if (rc) return rc;
    }
    return finish(c, s);  // the owners keep their scratch until everybody has pulled
}

// MPI_Scan (exclusive = false) / MPI_Exscan (true) in coll/basic's order (see the file header).
// sbuf NULL = MPI_IN_PLACE.  Exscan leaves rank 0's rbuf untouched.
// three: coll/libnbc's form of the same chain (MPI_Iscan / MPI_Iexscan under NB_ORDER = 1,
// nbc_iscan.c:89-105, nbc_iexscan.c:94-135): every step op3(in1 = own data, in2 = the partial).
// Messages of at least scan_part_min bytes per rank take the partitioned flow (scan_part) when
// the slot has a fold kernel and the buffers can be mapped; everything else the chain below.
static int scan_impl(mi355x_comm *c, const void *sbuf, void *rbuf, size_t count, int type, int op, bool exclusive,
                     void *stream, bool three = false)
{
    int rc = check_common(c, op, type);
    if (rc) return rc;
    if (c->size > kMaxRanks) return set_error(MI355X_ERR_UNSUPPORTED, "communicator larger than %d ranks", kMaxRanks);
    if (count == 0) return MI355X_SUCCESS;
    hipStream_t s = resolve_stream(stream);
    CallStream call_stream(c, s);
    const size_t esz = mi355x_type_size(type);
    const int me = c->rank;
    const void *in = sbuf ? sbuf : rbuf;
    const int last = exclusive ? me - 1 : me;   // fold over ranks 0..last
    if (!coll_slot_supported(op, type)) {  // (no fold kernel carries the slot: gather-then-fold, coll_gfold.cpp)
        return gfold_scan(c, in, rbuf, count, type, op, last, s, three);
    }
    if (c->size > 1 && c->scan_part_min && count * esz >= c->scan_part_min) {
        bool staged = false;
        rc = scan_part(c, in, rbuf, count, type, op, exclusive, three, s, &staged);
        if (rc || !staged) return rc;
    }
    // in place, rbuf is also an input the later ranks read: the result goes to scratch first
    const bool via_scratch = !sbuf && last >= 0 && !(last == 0 && me == 0);
    if (via_scratch) {
        rc = ensure_scratch(c, count * esz);
        if (rc) return rc;
    }
    MI_HIP(hipStreamSynchronize(s));
    const void *mine[1] = {in};
    const uint64_t sig[4] = {exclusive ? 25u : 24u, count, ((uint64_t)type << 32) | (uint64_t)op, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    void *target = via_scratch ? c->scratch : rbuf;
    if (last == 0) {   // rank 0 of scan, rank 1 of exscan: a copy of x0
        MultiCopyArgs m;
        std::memset(&m, 0, sizeof(m));
        add_seg(m, P[0][0], target, count * esz);
        rc = copy_segments(c, m, s);
        if (rc) return rc;
    } else if (last > 0) {
        Program pr;
        pr.is_fold = true;
        for (int q = 0; q <= last; ++q) pr.order.push_back(q);
        pr.role_mask = 0;   // ompi_op_reduce(op, partial, x_k): the partial is `in`
        pr.three = three;   // (libnbc: op(recvbuf = partial, sendbuf = x_k) -> in1 = x_k, in2 = partial)
        pr.nr = last + 1;
        std::vector<void *> dst(1, target);
        rc = run_program(op, type, pr, P[0], dst, 0, count, s);
        if (rc) return rc;
    }
    rc = finish(c, s);   // every rank has read every input
    if (rc) return rc;
    if (via_scratch) {
        MI_HIP(hipMemcpyAsync(rbuf, c->scratch, count * esz, hipMemcpyDeviceToDevice, s));
        MI_HIP(hipStreamSynchronize(s));
    }
    return MI355X_SUCCESS;
}

} // namespace mi355x

using namespace mi355x;

extern "C" {

int mi355x_gatherv(mi355x_comm_t *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                   const size_t *displs, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return gatherv_impl(c, sbuf, sbytes, rbuf, rcounts, displs, root, stream);
}

int mi355x_gather(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    std::vector<size_t> cnt((size_t)c->size, bytes), dsp((size_t)c->size);
    for (int q = 0; q < c->size; ++q) dsp[(size_t)q] = (size_t)q * bytes;
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return gatherv_impl(c, sbuf, bytes, rbuf, cnt.data(), dsp.data(), root, stream);
}

int mi355x_scatterv(mi355x_comm_t *c, const void *sbuf, const size_t *scounts, const size_t *displs, void *rbuf,
                    size_t rbytes, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return scatterv_impl(c, sbuf, scounts, displs, rbuf, rbytes, root, stream);
}

int mi355x_scatter(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    std::vector<size_t> cnt((size_t)c->size, bytes), dsp((size_t)c->size);
    for (int q = 0; q < c->size; ++q) dsp[(size_t)q] = (size_t)q * bytes;
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return scatterv_impl(c, sbuf, cnt.data(), dsp.data(), rbuf, bytes, root, stream);
}

int mi355x_allgatherv(mi355x_comm_t *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                      const size_t *displs, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return allgatherv_impl(c, sbuf, sbytes, rbuf, rcounts, displs, stream);
}

int mi355x_alltoallv(mi355x_comm_t *c, const void *sbuf, const size_t *scounts, const size_t *sdispls, void *rbuf,
                     const size_t *rcounts, const size_t *rdispls, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return alltoallv_impl(c, sbuf, scounts, sdispls, rbuf, rcounts, rdispls, stream);
}

int mi355x_gatherv_ddt(mi355x_comm_t *c, const void *sbuf, size_t sbytes, void *rbuf, const mi355x_ddt_t *rddt,
                       const size_t *rcounts, const size_t *rdispls, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    const RecvSide r(rddt, c->size, c->rank == root ? rcounts : nullptr, rdispls);
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return gatherv_impl(c, sbuf, sbytes, rbuf, r.counts, r.displs, root, stream, r.d);
}

int mi355x_scatterv_ddt(mi355x_comm_t *c, const void *sbuf, const size_t *scounts, const size_t *sdispls, void *rbuf,
                        const mi355x_ddt_t *rddt, size_t rcount, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    const RecvSide r(rddt, 1, &rcount, nullptr);
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return scatterv_impl(c, sbuf, scounts, sdispls, rbuf ? (char *)rbuf + r.first : rbuf, r.counts[0], root, stream, r.d);
}

int mi355x_allgatherv_ddt(mi355x_comm_t *c, const void *sbuf, size_t sbytes, void *rbuf, const mi355x_ddt_t *rddt,
                          const size_t *rcounts, const size_t *rdispls, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    const RecvSide r(rddt, c->size, rcounts, rdispls);
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return allgatherv_impl(c, sbuf, sbytes, rbuf, r.counts, r.displs, stream, r.d);
}

int mi355x_alltoallv_ddt(mi355x_comm_t *c, const void *sbuf, const size_t *scounts, const size_t *sdispls, void *rbuf,
                         const mi355x_ddt_t *rddt, const size_t *rcounts, const size_t *rdispls, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    const RecvSide r(rddt, c->size, rcounts, rdispls);
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return alltoallv_impl(c, sbuf, scounts, sdispls, rbuf, r.counts, r.displs, stream, r.d);
}

int mi355x_alltoall(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    std::vector<size_t> cnt((size_t)c->size, bytes), dsp((size_t)c->size);
    for (int q = 0; q < c->size; ++q) dsp[(size_t)q] = (size_t)q * bytes;
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return alltoallv_impl(c, sbuf, cnt.data(), dsp.data(), rbuf, cnt.data(), dsp.data(), stream);
}

int mi355x_scan(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return scan_impl(c, sbuf, rbuf, count, type, op, false, stream);
}

int mi355x_exscan(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    drain(c);
    CallGate gate(c);
    return scan_impl(c, sbuf, rbuf, count, type, op, true, stream);
}

int mi355x_iscan(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, void *stream,
                 mi355x_request_t **req)
{
    int rc = check_common(c, op, type);
    if (rc) return rc;
    const bool three = c->nb_order != 0;  // coll/libnbc's order (scan_impl)
    return post(c, stream, [=](hipStream_t s) { return scan_impl(c, sbuf, rbuf, count, type, op, false, s, three); }, req);
}

int mi355x_iexscan(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t count, int type, int op, void *stream,
                   mi355x_request_t **req)
{
    int rc = check_common(c, op, type);
    if (rc) return rc;
    const bool three = c->nb_order != 0;
    return post(c, stream, [=](hipStream_t s) { return scan_impl(c, sbuf, rbuf, count, type, op, true, s, three); }, req);
}

int mi355x_scan_part_plan(size_t count, int n, int q, int r, size_t *src_off, size_t *len, size_t *slot_off)
{
    if (n < 1 || n > kMaxRanks || q < 0 || q >= n || r < 0 || r >= n || !src_off || !len || !slot_off)
        return set_error(MI355X_ERR_ARG, "bad scan plan arguments");
    scan_part_plan(count, n, q, r, src_off, len, slot_off);
    return MI355X_SUCCESS;
}

int mi355x_ialltoall(mi355x_comm_t *c, const void *sbuf, void *rbuf, size_t bytes, void *stream,
                     mi355x_request_t **req)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    return post(c, stream,
                [=](hipStream_t s) {
                    std::vector<size_t> cnt((size_t)c->size, bytes), dsp((size_t)c->size);
                    for (int q = 0; q < c->size; ++q) dsp[(size_t)q] = (size_t)q * bytes;
                    return alltoallv_impl(c, sbuf, cnt.data(), dsp.data(), rbuf, cnt.data(), dsp.data(), s);
                },
                req);
}

} // extern "C"
