// coll_kernels.hip -- device side of coll/mi355x: one launch per rank per collective step that
// reads the ranks' inputs directly from IPC-mapped peer HBM over xGMI, folds them in the exact
// operand order of the reference schedule, and writes (pushes) the result into every
// destination -- local rbuf and/or the peers' rbufs.
//
// Three kernel families, instantiated per (MPI_Op, type) slot through the op functors:
//   k_fold  : acc = x[order[0]]; for j >= 1: acc = role[j] ? op2(out=acc, in=x[order[j]])
//                                                        : op2(out=x[order[j]], in=acc)
//             -- the ring / segmented-ring allreduce order (coll_tuned_allreduce.c:470-512,
//             acc is `in`), the pipeline / chain / linear reduce order (coll_tuned_reduce.c:
//             177-222, 687-703, acc is `out`), the ring reduce_scatter order.
//             All NR <= 8 loads of a vector are issued before the first op (one 16-B load per
//             rank per vector, U vectors in flight); ranks beyond 8 are folded in chunks,
//             which keeps the left-fold order.
//   k_tree  : a register program R[dst] = op2(out=R[o], in=R[i]) over <= 16 rank inputs --
//             the recursive-doubling butterfly (:193-284), binomial / binary reduce trees.
//   k_scan_part : every prefix of the rank chain (MPI_Scan / MPI_Exscan) in one pass: a running
//             accumulator per element, one destination per rank, k_fold's load chunks.
//   k_copy  : no arithmetic (allgather, bcast slices): one source, many destinations.
// k_fold, k_tree and k_ring_all also have a 3-buff form (template parameter THREE: op3(in1, in2) in
// place of op2(out, in)) for coll/libnbc's programs (Program::three, coll_nbc.cpp), and k_ring_all a
// form over libnbc's ring partition; the op2 instantiations are the code they were without them.
// Source/destination pointers arrive in the kernarg segment (uniform, scalar-loaded), so the
// per-rank indirection costs no VGPRs.  Same alignment scheme as op_kernels.hip: if every
// pointer shares the misalignment mod 16 a scalar head peels to the 16-B body, else the whole
// range runs element-wise.  The split, the vector access, the ordered fold (load_chunk /
// fold_chunk / store_vecs) and the launch plumbing are stream_core.hpp's, shared with
// op_kernels.hip and coll_pipe.hip.
#include "coll_internal.hpp"
#include "op_functors.hpp"
#include "rt_internal.hpp"
#include "slot_list.hpp"
#include "stream_core.hpp"

namespace mi355x {

// ------------------------------------------------------------------ fold
template <class F, int U, bool NT, bool THREE>
__global__ __launch_bounds__(256) void k_fold(FoldArgs a)
{
    using T = typename F::T;
    using V = Vec16<T>;
    constexpr int EPV = 16 / sizeof(T);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;

    for (size_t i = tid; i < a.head; i += nthr) {
        const T r = fold_scalar<F, THREE>(a.src, a.order, a.role_mask, a.nr, i);
        for (int d = 0; d < a.nd; ++d) static_cast<T *>(a.dst[d])[i] = r;
    }

    const size_t nvec = a.nvec;
    const size_t hb = a.head * sizeof(T);
    for (size_t base = tid; base < nvec; base += nthr * U) {
        V acc[U];
        // up to 8 ranks at a time: issue every load, then fold; the chunks keep the order.  The
        // first chunk stays peeled: as one loop the kernel needs fewer registers, but nine ranks
        // sharing a GPU ran 256 MiB per rank 1.5x slower (profiles/stream_core_speed.json)
        {
            V x[kFoldChunk][U];
            load_chunk<NT, V>(x, a.src, a.order, hb, 0, a.nr, base, nthr, nvec);
            fold_chunk<F, THREE>(acc, x, 0, a.nr, a.role_mask);
        }
        for (int j0 = kFoldChunk; j0 < a.nr; j0 += kFoldChunk) {
            V x[kFoldChunk][U];
            load_chunk<NT, V>(x, a.src, a.order, hb, j0, a.nr, base, nthr, nvec);
            fold_chunk<F, THREE>(acc, x, j0, a.nr, a.role_mask);
        }
        for (int d = 0; d < a.nd; ++d) store_vecs<NT>(static_cast<char *>(a.dst[d]) + hb, acc, base, nthr, nvec);
    }

    const size_t t0 = a.head + nvec * EPV;
    for (size_t i = t0 + tid; i < a.n; i += nthr) {
        const T r = fold_scalar<F, THREE>(a.src, a.order, a.role_mask, a.nr, i);
        for (int d = 0; d < a.nd; ++d) static_cast<T *>(a.dst[d])[i] = r;
    }
}

// ------------------------------------------------------------------ rank-chain prefixes, one pass
// MPI_Scan / MPI_Exscan over the elements one rank owns: one running accumulator per element
// yields every rank's prefix in the chain's own order (acc is `in` / `in2` at every step, as
// coll/basic's ompi_op_reduce(op, partial, x_k) and libnbc's op(recvbuf, sendbuf, tmp)).  The
// prefix after step k goes to dst[k + exclusive].  dst[r] may alias src[r] (MPI_IN_PLACE), so every
// store to dst[r] comes, in program order, after the lane's load of x_r at the same position:
// inclusive, x_k is part of the value stored; exclusive, x_{k+1} is in the chunk of loads already
// issued, or -- when k closes a chunk -- the store is held back (`pend`) until the next chunk's
// loads have been issued.  dst[nr-1] of the exclusive form aliases an input nobody reads.
template <class F, bool THREE>
__device__ __forceinline__ void scan_scalar(const ScanArgs &a, int nl, size_t i)
{
    using T = typename F::T;
    T x = static_cast<const T *>(a.src[0])[i];
    T acc = x;
    for (int k = 0; k < nl; ++k) {
        T nx = x;
        if (k + 1 < nl) nx = static_cast<const T *>(a.src[k + 1])[i];  // before the store below
        if (k) acc = rule<F, THREE>(x, acc);
        static_cast<T *>(a.dst[k + a.exclusive])[i] = acc;
        x = nx;
    }
}

template <class F, int U, bool NT, bool THREE>
__global__ __launch_bounds__(256) void k_scan_part(ScanArgs a)
{
    using T = typename F::T;
    using V = Vec16<T>;
    constexpr int EPV = 16 / sizeof(T);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const int ex = a.exclusive ? 1 : 0;
    const int nl = a.nr - ex;  // sources loaded
    if (nl <= 0) return;

    for (size_t i = tid; i < a.head; i += nthr) scan_scalar<F, THREE>(a, nl, i);

    const size_t nvec = a.nvec;
    const size_t hb = a.head * sizeof(T);
    for (size_t base = tid; base < nvec; base += nthr * U) {
        V acc[U];
        int pend = -1;  // destination whose store waits for the next chunk's loads
        for (int j0 = 0; j0 < nl; j0 += kFoldChunk) {
            V x[kFoldChunk][U];
            load_chunk<NT, V>(x, a.src, nullptr, hb, j0, nl, base, nthr, nvec);
            if (pend >= 0) {
                store_vecs<NT>(static_cast<char *>(a.dst[pend]) + hb, acc, base, nthr, nvec);
                pend = -1;
            }
#pragma unroll
            for (int j = 0; j < kFoldChunk; ++j) {
                const int k = j0 + j;
                if (k < nl) {
                    if (k == 0) {
#pragma unroll
                        for (int u = 0; u < U; ++u) acc[u] = x[0][u];
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u)
#pragma unroll
                            for (int e = 0; e < EPV; ++e) acc[u].e[e] = rule<F, THREE>(x[j][u].e[e], acc[u].e[e]);
                    }
                    // exclusive: x_{k+1} is loaded when it shares this chunk; when there is none
                    // (k + 1 == nl) the destination aliases no input that is read
                    if (!ex || j + 1 < kFoldChunk || k + 1 >= nl) {
                        store_vecs<NT>(static_cast<char *>(a.dst[k + ex]) + hb, acc, base, nthr, nvec);
                    } else {
                        pend = k + ex;
                    }
                }
            }
        }
    }

    const size_t t0 = a.head + nvec * EPV;
    for (size_t i = t0 + tid; i < a.n; i += nthr) scan_scalar<F, THREE>(a, nl, i);
}

// ------------------------------------------------------------------ ring order, whole vector
// Small ring-ordered messages: every rank evaluates every block (one element per lane, the n loads
// issued before the fold), so the allreduce needs one launch and one host barrier instead of two.
// NBC: coll/libnbc's ring instead (RingAllArgs::seg): element i of segment e = i / seg folds from
// rank e - 1 on; THREE as above.
template <class F, bool NBC, bool THREE> __global__ __launch_bounds__(256) void k_ring_all(RingAllArgs a)
{
    using T = typename F::T;
    const uint32_t se = a.split * a.early;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.count; i += gridDim.x * blockDim.x) {
        int b;
        if constexpr (NBC) {
            const int e = (int)(i / a.seg);  // < n: seg = ceil(count / n)
            b = e ? e - 1 : a.n - 1;
        } else {
            b = (int)(i < se ? i / a.early : a.split + (i - se) / a.late);
        }
        T acc{};
        for (int j0 = 0; j0 < a.n; j0 += kFoldChunk) {  // up to 8 loads in flight, then fold them
            T x[kFoldChunk];
#pragma unroll
            for (int j = 0; j < kFoldChunk; ++j) {
                const int jj = j0 + j, r = b + jj < a.n ? b + jj : b + jj - a.n;
                if (jj < a.n) x[j] = static_cast<const T *>(a.src[r])[i];
            }
#pragma unroll
            for (int j = 0; j < kFoldChunk; ++j) {
                if (j0 + j < a.n) acc = (j0 + j == 0) ? x[0] : rule<F, THREE>(x[j], acc);
            }
        }
        static_cast<T *>(a.dst)[i] = acc;
    }
}

// ------------------------------------------------------------------ tree program
template <class F>
__device__ __forceinline__ typename F::T pick(const typename F::T (&R)[kTreeMax], int k)
{
    typename F::T v = R[0];
#pragma unroll
    for (int s = 1; s < kTreeMax; ++s)
        if (s == k) v = R[s];
    return v;
}

template <class F, bool THREE> __global__ __launch_bounds__(256) void k_tree(TreeArgs a)
{
    using T = typename F::T;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < a.n; i += nthr) {
        T R[kTreeMax];
#pragma unroll
        for (int s = 0; s < kTreeMax; ++s)
            if (s < a.nr) R[s] = static_cast<const T *>(a.src[s])[i];
        for (int k = 0; k < a.nsteps; ++k) {
            const TreeStep st = a.steps[k];
            const T r = rule<F, THREE>(pick<F>(R, st.out), pick<F>(R, st.in));
#pragma unroll
            for (int s = 0; s < kTreeMax; ++s)
                if (s == st.dst) R[s] = r;
        }
        const T res = pick<F>(R, a.result);
        for (int d = 0; d < a.nd; ++d) static_cast<T *>(a.dst[d])[i] = res;
    }
}

// ------------------------------------------------------------------ copy (no arithmetic)
__global__ __launch_bounds__(256) void k_copy(CopyArgs a)
{
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)gridDim.x * blockDim.x;
    const char *s = static_cast<const char *>(a.src);
    for (size_t i = tid; i < a.head; i += nthr)
        for (int d = 0; d < a.nd; ++d) static_cast<char *>(a.dst[d])[i] = s[i];
    const size_t nvec = a.nvec;
    constexpr int U = 4;
    for (size_t base = tid; base < nvec; base += nthr * U) {
        u32x4 x[U];
        load_vecs<false>(x, s + a.head, base, nthr, nvec);
        for (int d = 0; d < a.nd; ++d) store_vecs<false>(static_cast<char *>(a.dst[d]) + a.head, x, base, nthr, nvec);
    }
    for (size_t i = a.head + nvec * 16 + tid; i < a.n; i += nthr)
        for (int d = 0; d < a.nd; ++d) static_cast<char *>(a.dst[d])[i] = s[i];
}

// ------------------------------------------------------------------ multi-segment copy
template <bool NT> __global__ __launch_bounds__(256) void k_multicopy(MultiCopyArgs a)
{
    // find this block's segment (<= 64 segments, uniform per block)
    int sgi = 0;
    while (sgi + 1 < a.nseg && blockIdx.x >= a.first_block[sgi + 1]) ++sgi;
    const unsigned nb = a.first_block[sgi + 1] - a.first_block[sgi];
    const unsigned b = blockIdx.x - a.first_block[sgi];
    const char *s = static_cast<const char *>(a.src[sgi]);
    char *d = static_cast<char *>(a.dst[sgi]);
    const size_t n = a.len[sgi];
    const size_t tid = (size_t)b * blockDim.x + threadIdx.x;
    const size_t nthr = (size_t)nb * blockDim.x;
    const uintptr_t ms = (uintptr_t)s & 15, md = (uintptr_t)d & 15;
    const Split16 sp = split16(n, 1, ms, ms == md);
    const size_t head = sp.head, nvec = sp.nvec;
    for (size_t i = tid; i < head; i += nthr) d[i] = s[i];
    constexpr int U = 4;
    for (size_t base = tid; base < nvec; base += nthr * U) {
        u32x4 x[U];
        load_vecs<NT>(x, s + head, base, nthr, nvec);
        store_vecs<NT>(d + head, x, base, nthr, nvec);
    }
    for (size_t i = head + nvec * 16 + tid; i < n; i += nthr) d[i] = s[i];
}

// ------------------------------------------------------------------ launchers
template <class F> static int launch_fold(FoldArgs a, hipStream_t s)
{
    using T = typename F::T;
    constexpr size_t EPV = 16 / sizeof(T);
    if (a.n == 0) return MI355X_SUCCESS;
    // the pointers the kernel touches: the fold's first source, every source, every destination
    const void *ptrs[1 + 2 * kMaxRanks];
    int np = 0;
    ptrs[np++] = a.src[a.order[0]];
    for (int j = 0; j < a.nr; ++j) ptrs[np++] = a.src[j];
    for (int d = 0; d < a.nd; ++d) ptrs[np++] = a.dst[d];
    const Split16 sp = split16(a.n, sizeof(T), (uintptr_t)ptrs[0] & 15, co_aligned(sizeof(T), ptrs, np));
    a.head = sp.head;
    a.nvec = sp.nvec;
    constexpr int U = 2;
    const dim3 grid((unsigned)grid_for_split(sp, a.n, EPV, U, coll_tune().blocks_per_cu));
    with_nt_three<F>(beyond_mall((size_t)(a.nr + a.nd) * a.n * sizeof(T)), a.three != 0, [&](auto nt, auto three) {
        hipLaunchKernelGGL((k_fold<F, U, nt, three>), grid, dim3(256), 0, s, a);
    });
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

template <class F> static int launch_scan(ScanArgs a, hipStream_t s)
{
    using T = typename F::T;
    constexpr size_t EPV = 16 / sizeof(T);
    const int ex = a.exclusive ? 1 : 0, nl = a.nr - ex;
    if (a.n == 0 || nl <= 0) return MI355X_SUCCESS;
    if (a.nr > kMaxRanks) return set_error(MI355X_ERR_UNSUPPORTED, "scan over more than %d ranks", kMaxRanks);
    // the pointers the kernel touches: sources 0..nl-1, destinations ex..nr-1
    const void *ptrs[2 * kMaxRanks];
    int np = 0;
    for (int j = 0; j < nl; ++j) ptrs[np++] = a.src[j];
    for (int d = ex; d < a.nr; ++d) ptrs[np++] = a.dst[d];
    const Split16 sp = split16(a.n, sizeof(T), (uintptr_t)ptrs[0] & 15, co_aligned(sizeof(T), ptrs, np));
    a.head = sp.head;
    a.nvec = sp.nvec;
    constexpr int U = 2;
    const dim3 grid((unsigned)grid_for_split(sp, a.n, EPV, U, coll_tune().blocks_per_cu));
    with_nt_three<F>(beyond_mall((size_t)(2 * nl) * a.n * sizeof(T)), a.three != 0, [&](auto nt, auto three) {
        hipLaunchKernelGGL((k_scan_part<F, U, nt, three>), grid, dim3(256), 0, s, a);
    });
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

template <class F> static int launch_ring_all(const RingAllArgs &a, hipStream_t s)
{
    if (a.count == 0) return MI355X_SUCCESS;
    const dim3 grid((unsigned)grid_for(a.count, 8));
    if (a.seg) {
        if constexpr (Op3Differs<F>::value) hipLaunchKernelGGL((k_ring_all<F, true, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_ring_all<F, true, false>), grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_ring_all<F, false, false>), grid, dim3(256), 0, s, a);
    }
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

template <class F> static int launch_tree(const TreeArgs &a, hipStream_t s)
{
    if (a.n == 0) return MI355X_SUCCESS;
    const dim3 grid((unsigned)grid_for(a.n, 4));
    with_three<F>(a.three != 0, [&](auto three) { hipLaunchKernelGGL((k_tree<F, three>), grid, dim3(256), 0, s, a); });
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

int launch_copy(CopyArgs a, hipStream_t s)
{
    if (a.n == 0) return MI355X_SUCCESS;
    const void *ptrs[1 + kMaxRanks];
    int np = 0;
    ptrs[np++] = a.src;
    for (int d = 0; d < a.nd; ++d) ptrs[np++] = a.dst[d];
    const Split16 sp = split16(a.n, 1, (uintptr_t)a.src & 15, co_aligned(1, ptrs, np));
    a.head = sp.head;
    a.nvec = sp.nvec;
    const size_t blocks = grid_for_split(sp, a.n, 16, 4, coll_tune().blocks_per_cu);  // k_copy's U
    hipLaunchKernelGGL(k_copy, dim3((unsigned)blocks), dim3(256), 0, s, a);
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

int launch_multicopy(MultiCopyArgs a, hipStream_t s)
{
    size_t total = 0;
    for (int i = 0; i < a.nseg; ++i) total += a.len[i];
    if (total == 0) return MI355X_SUCCESS;
    // copy_block_kib per block (default 4 KiB: one 16-B vector per lane); at most
    // blocks_per_cu x CUs blocks overall (beyond that the blocks loop)
    const size_t cap = (size_t)coll_tune().blocks_per_cu * (size_t)device_cu_count();
    unsigned next = 0;
    for (int i = 0; i < a.nseg; ++i) {
        a.first_block[i] = next;
        const size_t cb = (size_t)coll_tune().copy_block_kib << 10;
        size_t want = (a.len[i] + cb - 1) / cb;
        size_t share = total ? (cap * a.len[i] + total - 1) / total : 1;
        size_t nb = want < share ? want : share;
        if (a.len[i] && nb == 0) nb = 1;
        next += (unsigned)nb;
    }
    a.first_block[a.nseg] = next;
    if (next == 0) return MI355X_SUCCESS;
    if (beyond_mall(2 * total))
        hipLaunchKernelGGL(k_multicopy<true>, dim3(next), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_multicopy<false>, dim3(next), dim3(256), 0, s, a);
    MI_HIP(hipGetLastError());
    return MI355X_SUCCESS;
}

// dispatch table (same slot set as op_kernels.hip)
struct CollSlot {
    int (*fold)(FoldArgs, hipStream_t) = nullptr;
    int (*tree)(const TreeArgs &, hipStream_t) = nullptr;
    int (*ring_all)(const RingAllArgs &, hipStream_t) = nullptr;
    int (*scan)(ScanArgs, hipStream_t) = nullptr;
};

struct CollTable {
    CollSlot s[MI355X_OP_MAX_][MI355X_T_MAX];
    CollTable()
    {
        for_each_slot([&](auto tag, int op, int ty) {
            using F = typename decltype(tag)::type;
            s[op][ty].fold = &launch_fold<F>;
            s[op][ty].tree = &launch_tree<F>;
            s[op][ty].ring_all = &launch_ring_all<F>;
            s[op][ty].scan = &launch_scan<F>;
        });
    }
};

static const CollSlot *cslot(int op, int type)
{
    static const CollTable t;
    if (op < 0 || op >= MI355X_OP_MAX_ || type < 0 || type >= MI355X_T_MAX) return nullptr;
    const CollSlot *s = &t.s[op][type];
    return s->fold ? s : nullptr;
}

int launch_fold_slot(int op, int type, const FoldArgs &a, hipStream_t s)
{
    const CollSlot *sl = cslot(op, type);
    if (!sl) return set_error(MI355X_ERR_UNSUPPORTED, "no device fold for op %d type %d", op, type);
    return sl->fold(a, s);
}

int launch_scan_slot(int op, int type, const ScanArgs &a, hipStream_t s)
{
    const CollSlot *sl = cslot(op, type);
    if (!sl) return set_error(MI355X_ERR_UNSUPPORTED, "no device scan for op %d type %d", op, type);
    return sl->scan(a, s);
}

int launch_ring_all_slot(int op, int type, const RingAllArgs &a, hipStream_t s)
{
    const CollSlot *sl = cslot(op, type);
    if (!sl) return set_error(MI355X_ERR_UNSUPPORTED, "no device ring fold for op %d type %d", op, type);
    return sl->ring_all(a, s);
}

int launch_tree_slot(int op, int type, const TreeArgs &a, hipStream_t s)
{
    const CollSlot *sl = cslot(op, type);
    if (!sl) return set_error(MI355X_ERR_UNSUPPORTED, "no device tree for op %d type %d", op, type);
    return sl->tree(a, s);
}

bool coll_slot_supported(int op, int type) { return cslot(op, type) != nullptr; }

} // namespace mi355x

// every op/hip slot: the fold families' (slot_list.hpp) directly, the others gather-then-fold (coll_gfold.cpp)
extern "C" int mi355x_comm_op_supported(int op, int type) { return mi355x_op_supported(op, type); }
