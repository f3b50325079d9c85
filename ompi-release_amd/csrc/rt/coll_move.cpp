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

static int rows2_table(mi355x_comm *c, Rows2Table *t);

// ddt_unpack_segments for this communicator: its launch count and -- under MOVE_ROW_LEVELS = 2, and
// only where the layout can use it (rows of the normal form that are not one run per block) -- its
// piece table, which puts all pieces into one launch
static int unpack_segments(mi355x_comm *c, const mi355x_ddt *rddt, const void *const *src, void *const *mem,
                           const size_t *len, int nseg, hipStream_t s)
{
    Rows2Table tab{nullptr, nullptr};
    const bool levels = c->move_row_levels >= 2 && mi355x_ddt_nruns(rddt) != 1 && mi355x_ddt_row_levels(rddt) != 0;
    if (levels) {
        const int rc = rows2_table(c, &tab);
        if (rc) return rc;
    }
    return ddt_unpack_segments(rddt, src, mem, len, nseg, s, levels ? &tab : nullptr, &c->move_pull_launches);
}

// The pull.  Plain bytes: k_multicopy.  With a receive layout (the _ddt forms) the segments' bytes
// are packed streams of `rddt`, each unpacked from where it lies -- the owner's memory -- into the
// layout at its destination (ddt_unpack_segments): no dense receive view, no second pass.
static int copy_segments(mi355x_comm *c, MultiCopyArgs &m, hipStream_t s, const mi355x_ddt *rddt = nullptr)
{
    if (m.nseg == 0) return MI355X_SUCCESS;
    if (!rddt) {
        c->move_pull_launches++;
        return launch_multicopy(m, s);
    }
    c->move_fused++;
    return unpack_segments(c, rddt, m.src, m.dst, m.len, m.nseg, s);
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

// The send side of a _ddt2 form as the impls take it: byte counts and displacements, and -- when
// the layout is eligible (move_send_direct_ok) -- the rows this rank publishes instead of packing.
// A NULL layout, or counts that are not significant here, is the _ddt form's send side (bytes); a
// layout without gaps becomes bytes as RecvSide's does; any other layout that fails the rule sets rc
// (MI355X_ERR_UNSUPPORTED: the caller packs), before the rank meets anybody.
struct SendSide {
    const RowLay *lay = nullptr;  // the published rows (NULL: dense bytes)
    const size_t *counts, *displs;
    int64_t first = 0;            // a gap-free layout's first byte (in displs already)
    int rc = MI355X_SUCCESS;
    RowLay rows{};
    std::vector<size_t> bytes;
    SendSide(mi355x_comm *c, const char *call, const void *sbuf, const mi355x_ddt *sddt, int n, const size_t *cnt,
             const size_t *dsp)
        : counts(cnt), displs(dsp)
    {
        if (!sddt || !cnt) return;
        const SendShape sh = ddt_send_shape(sddt, c->move_row_levels);
        size_t most = 0;
        for (int q = 0; q < n; ++q) most = std::max(most, cnt[q]);
        const bool gap_free = send_gap_free(sh, most);
        if (!gap_free && !move_send_direct_ok(sh, cnt, nullptr, n, sbuf == nullptr, (int64_t)c->move_send_min_run)) {
            rc = set_error(MI355X_ERR_UNSUPPORTED, "%s: the send layout is not pulled from directly (%d runs per block, run %lld B, "
                           "MOVE_SEND_MIN_RUN %zu, MOVE_ROW_LEVELS %d%s): pack it", call, sh.nruns, (long long)sh.lay.run,
                           c->move_send_min_run, c->move_row_levels, sbuf ? "" : ", MPI_IN_PLACE");
            return;
        }
        bytes.resize(2 * (size_t)n);
        size_t reach = 0;
        for (int q = 0; q < n; ++q) {
            const size_t at = dsp ? dsp[q] : 0;
            bytes[(size_t)q] = cnt[q] * (size_t)sh.size;
            bytes[(size_t)(n + q)] = at + (gap_free ? (size_t)sh.lay.disp : 0);
            if (cnt[q])
                reach = std::max(reach, at + (size_t)((int64_t)(cnt[q] - 1) * sh.lay.extent + (sh.lay.n1 - 1) * sh.lay.step1 +
                                                      (sh.lay.nblk - 1) * sh.lay.stride + sh.lay.disp + sh.lay.run));
        }
        counts = bytes.data();
        if (dsp) displs = bytes.data() + n;
        if (gap_free) {
            first = sh.lay.disp;
            return;
        }
        rc = check_in_allocation(c, sbuf, reach, call);
        rows = sh.lay;
        lay = &rows;
    }
};

// what this rank's published buffer holds for its peers: dense bytes, or the rows of `lay`
static void publish_layout(mi355x_comm *c, const RowLay *lay)
{
    c->ctrl->slot[c->rank].slay = lay ? *lay : row_dense();
}

// The pieces of one rank's pull: k_multicopy's segments, and beside each the layout its owner
// published for it.
struct Pull {
    MultiCopyArgs m;
    RowLay sl[kMaxSegs];
    bool rows = false;  // some piece is read through a send layout
    Pull() { std::memset(&m, 0, sizeof(m)); }
};

static int add_piece(Pull &p, const void *src, const RankSlot &owner, void *dst, size_t len)
{
    const RowLay &l = owner.slay;
    if (len == 0 || (l.nblk == 0 && src == dst)) return MI355X_SUCCESS;
    if (l.nblk < 0 || (l.nblk && (l.run <= 0 || l.disp < 0 || l.nblk >= ((int64_t)1 << 32) || l.run >= ((int64_t)1 << 32) ||
                                  l.n1 < 1 || l.n1 >= ((int64_t)1 << 32))))
        return set_error(MI355X_ERR_PEER, "a peer published a send layout this rank cannot read");
    p.m.src[p.m.nseg] = src;
    p.m.dst[p.m.nseg] = dst;
    p.m.len[p.m.nseg] = len;
    p.sl[p.m.nseg] = l;
    p.rows = p.rows || l.nblk != 0;
    p.m.nseg++;
    return MI355X_SUCCESS;
}

// the two-ended row gather's piece table, made at the first pull that needs one
static int rows2_table(mi355x_comm *c, Rows2Table *t)
{
    if (!c->rows2_dev) MI_HIP(hipMalloc(&c->rows2_dev, kRows2TableBytes));
    if (!c->rows2_host) MI_HIP(hipHostMalloc(&c->rows2_host, kRows2TableBytes, hipHostMallocDefault));
    t->dev = c->rows2_dev;
    t->host = c->rows2_host;
    return MI355X_SUCCESS;
}

// The pull, whatever the owners published.  No send layout among the pieces: copy_segments, the
// kernels of the plain and _ddt forms.  Otherwise one launch of the two-ended row gather
// (ddt_gather_segments) for all pieces, dense ones included, into rddt or dense bytes.  When that
// declines -- rddt is a run list (or rows that this rank's MOVE_ROW_LEVELS keeps off the launch), or
// an end is beyond the 32-bit slot arithmetic -- the
// dense pieces take copy_segments' kernels and the row pieces a launch of their own; and when rddt
// is what it cannot take, the row pieces are gathered into the scratch as dense bytes (a dense
// destination always applies to what move_send_direct_ok let a sender publish) and unpacked from
// there (ddt_unpack_segments, as a _ddt form unpacks a peer's dense bytes).
static int pull_segments(mi355x_comm *c, Pull &p, hipStream_t s, const mi355x_ddt *rddt)
{
    if (!p.rows) return copy_segments(c, p.m, s, rddt);
    if (rddt) c->move_fused++;
    Rows2Table tab;
    int rc = rows2_table(c, &tab);
    if (rc) return rc;
    const int n = p.m.nseg;
    Row2Seg all[kMaxSegs];
    for (int i = 0; i < n; ++i) all[i] = Row2Seg{p.m.src[i], p.sl[i], p.m.dst[i], p.m.len[i]};
    rc = ddt_gather_segments(rddt, all, n, tab, s, c->move_row_levels, &c->move_pull_launches);
    if (rc != 1) return rc;
    MultiCopyArgs dn;
    std::memset(&dn, 0, sizeof(dn));
    Row2Seg rw[kMaxSegs];
    int nr = 0;
    for (int i = 0; i < n; ++i) {
        if (p.sl[i].nblk) rw[nr++] = all[i];
        else add_seg(dn, p.m.src[i], p.m.dst[i], p.m.len[i]);
    }
    if (dn.nseg) {
        if (!rddt) c->move_pull_launches++;
        rc = rddt ? unpack_segments(c, rddt, dn.src, dn.dst, dn.len, dn.nseg, s) : launch_multicopy(dn, s);
        if (rc) return rc;
    }
    rc = ddt_gather_segments(rddt, rw, nr, tab, s, c->move_row_levels, &c->move_pull_launches);
    if (rc != 1) return rc;
    if (!rddt) return set_error(MI355X_ERR_UNSUPPORTED, "a published send layout is beyond the row gather's limits");
    // two passes.  (The scratch is free: only alltoallv in place publishes it, and in place takes no rddt)
    size_t total = 0;
    const void *dsrc[kMaxSegs];
    void *dmem[kMaxSegs];
    size_t dlen[kMaxSegs];
    for (int i = 0; i < nr; ++i) total += (rw[i].len + 15) & ~(size_t)15;
    rc = ensure_scratch(c, total);
    if (rc) return rc;
    total = 0;
    for (int i = 0; i < nr; ++i) {
        dmem[i] = rw[i].mem;
        dlen[i] = rw[i].len;
        rw[i].mem = (char *)c->scratch + total;
        dsrc[i] = rw[i].mem;
        total += (rw[i].len + 15) & ~(size_t)15;
    }
    rc = ddt_gather_segments(nullptr, rw, nr, tab, s, c->move_row_levels, &c->move_pull_launches);
    if (rc == 1) rc = set_error(MI355X_ERR_UNSUPPORTED, "a published send layout is beyond the row gather's limits");
    if (rc) return rc;
    return unpack_segments(c, rddt, dsrc, dmem, dlen, nr, s);
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
// slay (every impl below): NULL, or the rows this rank's send counts are read through -- the counts
// stay bytes of the packed stream; the rank publishes sbuf itself and the record beside the counts.
static int gatherv_impl(mi355x_comm *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                        const size_t *displs, int root, void *stream, const mi355x_ddt *rddt = nullptr,
                        const RowLay *slay = nullptr)
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
    publish_layout(c, slay);
    const void *mine[1] = {sbytes ? sbuf : nullptr};
    const uint64_t sig[4] = {20, (uint64_t)root, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    if (slay && mine[0]) c->move_send_direct++;
    if (am_root) {
        Pull m;
        for (int q = 0; q < c->size; ++q) {
            const size_t qb = (size_t)c->ctrl->slot[q].varg[0];
            if (qb > piece_bytes(rddt, rcounts[q]))
                return set_error(MI355X_ERR_TRUNCATE, "gatherv: rank %d sends %zu bytes, root expects %zu", q, qb,
                                 piece_bytes(rddt, rcounts[q]));
            if (qb && (rc = add_piece(m, P[0][q], c->ctrl->slot[q], (char *)rbuf + displs[q], qb))) return rc;
        }
        rc = pull_segments(c, m, s, rddt);
        if (rc) return rc;
    }
    return finish(c, s);
}

// MPI_Scatterv: rank r pulls scounts[r] bytes at root's sbuf + displs[r] (both published by the
// root) into rbuf (at most rbytes).  rbuf NULL at the root = MPI_IN_PLACE.
static int scatterv_impl(mi355x_comm *c, const void *sbuf, const size_t *scounts, const size_t *displs, void *rbuf,
                         size_t rbytes, int root, void *stream, const mi355x_ddt *rddt = nullptr,
                         const RowLay *slay = nullptr)
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
    if (!am_root) slay = nullptr;  // (no send side)
    publish_layout(c, slay);
    const void *mine[1] = {am_root && any ? sbuf : nullptr};
    const uint64_t sig[4] = {21, (uint64_t)root, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    if (slay && mine[0]) c->move_send_direct++;
    const RankSlot &rs = c->ctrl->slot[root];
    const size_t len = (size_t)rs.varg[c->rank];
    if (rbuf && len) {
        if (len > piece_bytes(rddt, rbytes))
            return set_error(MI355X_ERR_TRUNCATE, "scatterv: root sends %zu bytes to rank %d, which expects %zu", len,
                             c->rank, piece_bytes(rddt, rbytes));
        Pull m;
        rc = add_piece(m, (const char *)P[0][root] + rs.varg[kMaxRanks + c->rank], rs, rbuf, len);
        if (rc) return rc;
        rc = pull_segments(c, m, s, rddt);
        if (rc) return rc;
    }
    return finish(c, s);
}

// MPI_Allgatherv: every rank pulls rank q's block (rcounts[q] bytes) into rbuf + displs[q].
// sbuf NULL = MPI_IN_PLACE (the rank's block is at rbuf + displs[rank]).
static int allgatherv_impl(mi355x_comm *c, const void *sbuf, size_t sbytes, void *rbuf, const size_t *rcounts,
                           const size_t *displs, void *stream, const mi355x_ddt *rddt = nullptr,
                           const RowLay *slay = nullptr)
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
    publish_layout(c, slay);
    const void *mine[1] = {mybytes ? src : nullptr};
    const uint64_t sig[4] = {22, 0, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    if (slay && mine[0]) c->move_send_direct++;
    Pull m;
    for (int q = 0; q < c->size; ++q)
        if (rcounts[q] && P[0][q]) {
            rc = add_piece(m, P[0][q], c->ctrl->slot[q], (char *)rbuf + displs[q], q == me ? mybytes : piece_bytes(rddt, rcounts[q]));
            if (rc) return rc;
        }
    rc = pull_segments(c, m, s, rddt);
    if (rc) return rc;
    return finish(c, s);
}

// MPI_Alltoallv: rank r pulls from rank q the scounts_q[r] bytes at q's sbuf + sdispls_q[r]
// (published by q) into rbuf + rdispls[q] (at most rcounts[q]).  sbuf NULL = MPI_IN_PLACE: the
// data to send is rbuf laid out by rcounts / rdispls, snapshotted into scratch first.
static int alltoallv_impl(mi355x_comm *c, const void *sbuf, const size_t *scounts, const size_t *sdispls, void *rbuf,
                          const size_t *rcounts, const size_t *rdispls, void *stream, const mi355x_ddt *rddt = nullptr,
                          const RowLay *slay = nullptr)
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
    publish_layout(c, slay);
    const void *mine[1] = {any ? src : nullptr};
    const uint64_t sig[4] = {23, 0, 0, 0};
    std::vector<std::vector<void *>> P;
    rc = exchange(c, 1, mine, sig, P);
    if (rc) return rc;
    c->last_alg = 1;
    if (slay && mine[0]) c->move_send_direct++;
    Pull m;
    for (int k = 0; k < n; ++k) {
        const int q = (me + k) % n;   // own block first, then the peers in ring order
        const RankSlot &qs = c->ctrl->slot[q];
        const size_t len = (size_t)qs.varg[me];
        if (len > piece_bytes(rddt, rcounts[q]))
            return set_error(MI355X_ERR_TRUNCATE, "alltoallv: rank %d sends %zu bytes to rank %d, which expects %zu",
                             q, len, me, piece_bytes(rddt, rcounts[q]));
        if (len && (rc = add_piece(m, (const char *)P[0][q] + qs.varg[kMaxRanks + me], qs, (char *)rbuf + rdispls[q], len)))
            return rc;
    }
    rc = pull_segments(c, m, s, rddt);
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

// The _ddt2 forms: the _ddt forms with a send layout (SendSide).
int mi355x_gatherv_ddt2(mi355x_comm_t *c, const void *sbuf, const mi355x_ddt_t *sddt, size_t scount, void *rbuf,
                        const mi355x_ddt_t *rddt, const size_t *rcounts, const size_t *rdispls, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    const SendSide sn(c, "gatherv", sbuf, sddt, 1, &scount, nullptr);
    if (sn.rc) return sn.rc;
    const RecvSide r(rddt, c->size, c->rank == root ? rcounts : nullptr, rdispls);
    drain(c);
    CallGate gate(c);
    return gatherv_impl(c, sbuf ? (const char *)sbuf + sn.first : sbuf, sn.counts[0], rbuf, r.counts, r.displs, root, stream, r.d,
                        sn.lay);
}

int mi355x_scatterv_ddt2(mi355x_comm_t *c, const void *sbuf, const mi355x_ddt_t *sddt, const size_t *scounts,
                         const size_t *sdispls, void *rbuf, const mi355x_ddt_t *rddt, size_t rcount, int root, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    const bool am_root = c->rank == root;
    if (am_root && sddt && (!scounts || !sdispls)) return set_error(MI355X_ERR_ARG, "scatterv: counts at the root are NULL");
    // (in place at the root is rbuf NULL: the send side is significant and read by the others as usual)
    const SendSide sn(c, "scatterv", sbuf, am_root ? sddt : nullptr, c->size, scounts, sdispls);
    if (sn.rc) return sn.rc;
    const RecvSide r(rddt, 1, &rcount, nullptr);
    drain(c);
    CallGate gate(c);
    return scatterv_impl(c, sbuf, sn.counts, sn.displs, rbuf ? (char *)rbuf + r.first : rbuf, r.counts[0], root, stream, r.d,
                         sn.lay);
}

int mi355x_allgatherv_ddt2(mi355x_comm_t *c, const void *sbuf, const mi355x_ddt_t *sddt, size_t scount, void *rbuf,
                           const mi355x_ddt_t *rddt, const size_t *rcounts, const size_t *rdispls, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    const SendSide sn(c, "allgatherv", sbuf, sddt, 1, &scount, nullptr);
    if (sn.rc) return sn.rc;
    const RecvSide r(rddt, c->size, rcounts, rdispls);
    drain(c);
    CallGate gate(c);
    return allgatherv_impl(c, sbuf ? (const char *)sbuf + sn.first : sbuf, sn.counts[0], rbuf, r.counts, r.displs, stream, r.d,
                           sn.lay);
}

int mi355x_alltoallv_ddt2(mi355x_comm_t *c, const void *sbuf, const mi355x_ddt_t *sddt, const size_t *scounts,
                          const size_t *sdispls, void *rbuf, const mi355x_ddt_t *rddt, const size_t *rcounts,
                          const size_t *rdispls, void *stream)
{
    if (!c) return set_error(MI355X_ERR_ARG, "comm is NULL");
    DeviceGuard dg(c->device);
    if (sddt && sbuf && (!scounts || !sdispls)) return set_error(MI355X_ERR_ARG, "alltoallv: counts are NULL");
    // (in place the send arguments are not read: only a layout with gaps is refused, as rddt's is)
    if (sddt && !sbuf && !send_gap_free(ddt_send_shape(sddt, c->move_row_levels), 2))
        return set_error(MI355X_ERR_UNSUPPORTED, "alltoallv: MPI_IN_PLACE with a send layout");
    const SendSide sn(c, "alltoallv", sbuf, sbuf ? sddt : nullptr, c->size, scounts, sdispls);
    if (sn.rc) return sn.rc;
    const RecvSide r(rddt, c->size, rcounts, rdispls);
    drain(c);
    CallGate gate(c);
    return alltoallv_impl(c, sbuf, sn.counts, sn.displs, rbuf, r.counts, r.displs, stream, r.d, sn.lay);
}

int mi355x_move_send_direct_ok(const mi355x_comm_t *c, const mi355x_ddt_t *sddt, const size_t *scounts, int n)
{
    if (!c || !sddt || n < 0 || (n && !scounts)) return set_error(MI355X_ERR_ARG, "bad send layout arguments");
    return move_send_direct_ok(ddt_send_shape(sddt, c->move_row_levels), scounts, nullptr, n, false,
                               (int64_t)c->move_send_min_run) ? 1 : 0;
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
