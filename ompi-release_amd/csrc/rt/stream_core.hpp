// stream_core.hpp -- what the bandwidth kernels share: op/hip's k_stream / k_chunk
// (op_kernels.hip), the engine's k_fold / k_scan_part / k_copy / k_multicopy (coll_kernels.hip) and
// the pipelined allreduce (coll_pipe.hip); the LL service and the convertor take the vector type.
//   * the head / 16-B body / tail split of a range (Split16, split16, co_aligned): plain C++, so
//     tools/split16_check.cpp compiles it for the host alone;
//   * 16-byte vector access (u32x4, Vec16, vload / vstore, optionally non-temporal) and the
//     system-coherent cache policy of the raw buffer operations;
//   * the ordered fold over rank inputs: fold_step / fold_scalar, and the vector form in three
//     pieces -- load_chunk (issue the loads of up to FC ranks, U vectors per lane in flight),
//     fold_chunk (fold them left to right under role_mask), store_vecs (and load_vecs, the copies');
//   * launch plumbing: the (non-temporal, 3-buff) kernel choice, the grid of a split range, the
//     "beyond the Infinity Cache" test.
#pragma once

#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#ifndef MI_HD
#define MI_HD __host__ __device__ inline
#endif

namespace mi355x {

// ------------------------------------------------------------------ head / 16-B body / tail
// A range of n elements of esz bytes (esz divides 16) whose operands all sit m bytes past a 16-B
// boundary: `head` scalar elements reach the boundary, `nvec` whole 16-B vectors follow, the rest
// is the scalar tail.  Operands that are not co-aligned (or m is no whole element) take the whole
// range element-wise: head = n, nvec = 0.
struct Split16 {
    size_t head, nvec;
};

MI_HD Split16 split16(size_t n, size_t esz, uintptr_t m, bool co)
{
    Split16 s{n, 0};
    if (co && m % esz == 0) {
        s.head = m ? (16 - m) / esz : 0;
        if (s.head > n) s.head = n;
        s.nvec = (n - s.head) / (16 / esz);
    }
    return s;
}

// every pointer shares the first one's misalignment mod 16, and that is a whole element
inline bool co_aligned(size_t esz, const void *const *ptrs, int nptrs)
{
    const uintptr_t m = (uintptr_t)ptrs[0] & 15;
    bool co = (m % esz) == 0;
    for (int i = 1; i < nptrs && co; ++i) co = ((uintptr_t)ptrs[i] & 15) == m;
    return co;
}

// streams beyond the 256 MiB Infinity Cache run non-temporal (not allocating in L2 / MALL gains
// ~9 % there; small, re-read operands lose)
inline bool beyond_mall(size_t bytes) { return bytes > ((size_t)256 << 20); }

} // namespace mi355x

#ifdef __HIPCC__
#include <type_traits>

#include "op_functors.hpp"
#include "rt_internal.hpp"

namespace mi355x {

// ------------------------------------------------------------------ 16-byte vector access
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct alignas(16) Vec16 {
    T e[16 / sizeof(T)];
};

template <bool NT, typename V> __device__ __forceinline__ V vload(const void *p)
{
    u32x4 raw;
    if constexpr (NT)
        raw = __builtin_nontemporal_load(static_cast<const u32x4 *>(p));
    else
        raw = *static_cast<const u32x4 *>(p);
    V v;
    __builtin_memcpy(&v, &raw, 16);
    return v;
}

template <bool NT, typename V> __device__ __forceinline__ void vstore(void *p, const V &v)
{
    u32x4 raw;
    __builtin_memcpy(&raw, &v, 16);
    if constexpr (NT)
        __builtin_nontemporal_store(raw, static_cast<u32x4 *>(p));
    else
        *static_cast<u32x4 *>(p) = raw;
}

// gfx950 cache-policy bits of the raw buffer operations: sc0 (1) | sc1 (16), system coherent --
// loads skip the CU's L1, stores go through the XCD's L2 to memory
constexpr int kSysCoherent = 1 | 16;

// ------------------------------------------------------------------ the two reduction rules
// THREE: the 3-buff rule op3(in1 = o, in2 = a) of coll/libnbc's programs (Program::three) instead
// of the 2-buff rule op2(out = o, in = a).  The two differ for the MAXLOC / MINLOC pairs only
// (op_functors.hpp: a NaN value, the value kept on a tie), so only those slots instantiate the
// THREE kernels; every other slot's op3 is its op2 and a `three` program runs the op2 kernels.
template <class F> struct Op3Differs : std::false_type {};
template <typename P, bool MAX> struct Op3Differs<OpLoc<P, MAX>> : std::true_type {};

template <class F, bool THREE>
__device__ __forceinline__ typename F::T rule(const typename F::T &o, const typename F::T &a)
{
    if constexpr (THREE) return F::op3(o, a);
    else return F::op2(o, a);
}

// ------------------------------------------------------------------ ordered fold
// acc = x[order[0]]; step j >= 1: acc = role_mask bit j ? rule(out = acc, in = x[order[j]])
//                                                       : rule(out = x[order[j]], in = acc)
template <class F, bool THREE>
__device__ __forceinline__ typename F::T fold_step(const typename F::T &acc, const typename F::T &x,
                                                   bool acc_is_out)
{
    return acc_is_out ? rule<F, THREE>(acc, x) : rule<F, THREE>(x, acc);
}

// fold of element i (scalar path)
template <class F, bool THREE>
__device__ __forceinline__ typename F::T fold_scalar(const void *const *src, const int *order, uint64_t role_mask,
                                                     int nr, size_t i)
{
    using T = typename F::T;
    T acc = static_cast<const T *>(src[order[0]])[i];
    for (int j = 1; j < nr; ++j) {
        const T x = static_cast<const T *>(src[order[j]])[i];
        acc = fold_step<F, THREE>(acc, x, (role_mask >> j) & 1u);
    }
    return acc;
}

// The vector body: a lane holds vectors base, base + stride, ... (U of them, those below nvec) of
// the range that starts `off` bytes into every source.  load_chunk issues the loads of fold
// positions j0 .. j0 + FC - 1 (those below nr) before anything is folded; position j reads
// src[order[j]], or src[j] without an order.  L is the type the 16 bytes are loaded as before they
// are copied into x: V itself (k_fold, k_scan_part) or u32x4 (the pipelined kernel) -- the form each
// kernel had before the fold was shared; with it the kernels keep the scratch and occupancy they
// were measured with (profiles/stream_core_regs.tsv).
template <bool NT, typename L, int U, int FC, typename V>
__device__ __forceinline__ void load_chunk(V (&x)[FC][U], const void *const *src, const int *order, size_t off,
                                           int j0, int nr, size_t base, size_t stride, size_t nvec)
{
#pragma unroll
    for (int j = 0; j < FC; ++j) {
        if (j0 + j < nr) {
            const char *p = static_cast<const char *>(src[order ? order[j0 + j] : j0 + j]) + off;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const size_t v = base + (size_t)u * stride;
                if (v < nvec) {
                    const L raw = vload<NT, L>(p + v * 16);
                    __builtin_memcpy(&x[j][u], &raw, 16);
                }
            }
        }
    }
}

// fold a loaded chunk into acc, in order; position 0 initialises
template <class F, bool THREE, int U, int FC, typename V>
__device__ __forceinline__ void fold_chunk(V (&acc)[U], V (&x)[FC][U], int j0, int nr, uint64_t role_mask)
{
    constexpr int EPV = 16 / sizeof(typename F::T);
    if (j0 == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = x[0][u];
    }
#pragma unroll
    for (int j = 0; j < FC; ++j) {
        if (j0 + j > 0 && j0 + j < nr) {
            const bool ao = (role_mask >> (j0 + j)) & 1u;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < EPV; ++e) acc[u].e[e] = fold_step<F, THREE>(acc[u].e[e], x[j][u].e[e], ao);
        }
    }
}

// the lane's U vectors from one source (p: address of vector 0) ...
template <bool NT, int U, typename V>
__device__ __forceinline__ void load_vecs(V (&x)[U], const void *p, size_t base, size_t stride, size_t nvec)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const size_t v = base + (size_t)u * stride;
        if (v < nvec) x[u] = vload<NT, V>(static_cast<const char *>(p) + v * 16);
    }
}

// ... and to one destination (q: address of vector 0)
template <bool NT, int U, typename V>
__device__ __forceinline__ void store_vecs(void *q, const V (&x)[U], size_t base, size_t stride, size_t nvec)
{
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const size_t v = base + (size_t)u * stride;
        if (v < nvec) vstore<NT, V>(static_cast<char *>(q) + v * 16, x[u]);
    }
}

// ------------------------------------------------------------------ launch plumbing
// f(three) / f(nt, three) with the flags as compile-time constants (std::bool_constant); the
// THREE = true call is instantiated only for the functors whose op3 differs from op2, and `three`
// is ignored for the rest
template <class F, class Fn> void with_three(bool three, Fn &&f)
{
    if constexpr (Op3Differs<F>::value) {
        if (three) {
            f(std::true_type{});
            return;
        }
    }
    f(std::false_type{});
}

template <class F, class Fn> void with_nt_three(bool nt, bool three, Fn &&f)
{
    with_three<F>(three, [&](auto t) {
        if (nt) f(std::true_type{}, t);
        else f(std::false_type{}, t);
    });
}

// blocks of 256 lanes, one lane per unit of work: at most blocks_per_cu x CUs, at least one
inline size_t grid_for(size_t work, int blocks_per_cu)
{
    size_t blocks = (work + 255) / 256;
    const size_t cap = (size_t)blocks_per_cu * (size_t)device_cu_count();
    if (blocks > cap) blocks = cap;
    return blocks ? blocks : 1;
}

// a split range: a lane takes U vectors per pass or one scalar element, whichever needs more lanes
inline size_t grid_for_split(const Split16 &sp, size_t n, size_t epv, int U, int blocks_per_cu)
{
    size_t work = sp.nvec ? (sp.nvec + (size_t)U - 1) / U : 0;
    const size_t scalar = n - sp.nvec * epv;
    if (scalar > work) work = scalar;
    return grid_for(work, blocks_per_cu);
}

} // namespace mi355x
#endif // __HIPCC__
