// ddt_rows_plan.hpp -- the host side of the row kernels' launches (ddt_kernels.hip), plain C++ so
// tools/rows_plan_check.cpp compiles it for the host alone:
//   * rows_width: the slot width one window of a row layout (one run per block) can move with;
//   * plan_rows_multi: one launch unpacking several packed pieces into the same row layout (the pull
//     of a movement collective into a derived receive datatype): which pieces it keeps, the slot
//     width they share and the blocks each one gets;
//   * row_levels_view: a layout's run tables read as rows of up to two levels (the normal form);
//   * move_send_direct_ok: which send layouts a movement collective publishes instead of packing;
//   * plan_rows2_multi: the same plan for the two-ended row gather (k_ddt_rows2_multi), whose pieces
//     are read through a row layout of their own and written through the receiver's.
#pragma once

#include <cstddef>
#include <cstdint>

// the few functions a kernel shares with the host checks (the divisions and the slot mapping)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI355X_HD __host__ __device__ inline
#else
#define MI355X_HD inline
#endif

namespace mi355x {

// 32-bit division by a constant as a multiply-high and a shift (Granlund-Montgomery; the magic
// numbers are computed on the host once per launch): exact for every 32-bit n and d >= 1
struct FastDiv {
    uint32_t m, l, d;
};

inline FastDiv make_fastdiv(uint32_t d)
{
    FastDiv f;
    f.d = d;
    uint32_t l = 0;
    while (l < 32 && ((uint64_t)1 << l) < d) ++l;
    f.l = l;
    f.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
    return f;
}

MI355X_HD uint32_t fast_div(uint32_t n, const FastDiv &f)
{
    return (uint32_t)(((((uint64_t)f.m * n) >> 32) + n) >> f.l);
}

// largest slot index the 32-bit row / unit kernels take: their grid-stride and last-block index
// arithmetic (at most 2^22 slots past the end) must not wrap
constexpr int64_t kSlot32Max = ((int64_t)1 << 32) - ((int64_t)1 << 22);

// the slot width the row kernel can use (0: it does not apply): one run per block, and every
// address, length and window a multiple of W; slot / row counts in 32 bits
inline int rows_width(int64_t stride, int64_t extent, int64_t nblk, int nruns_host, int64_t run_disp, int64_t run_len,
                      const void *mem, const void *packed, int64_t pos, int64_t bytes)
{
    if (nruns_host != 1 || run_len <= 0) return 0;
    const uint64_t bits = (uint64_t)run_len | ((uintptr_t)mem + (uint64_t)run_disp) | (uint64_t)stride |
                          (uint64_t)extent | (uintptr_t)packed | (uint64_t)pos | (uint64_t)bytes;
    int w = 16;
    while (w > 1 && (bits & (uint64_t)(w - 1))) w >>= 1;
    const int64_t last_slot = (pos + bytes) / w;
    const int64_t rows = last_slot / (run_len / w) + 1;
    // 32-bit slot arithmetic, with headroom for the last block's (tpb x U)-slot stride
    if (last_slot >= kSlot32Max || rows >= ((int64_t)1 << 32) || nblk >= ((int64_t)1 << 32) ||
        (run_len / w) >= ((int64_t)1 << 32))
        return 0;
    return w;
}

// One launch, several pieces.  Piece i: `len` packed bytes at `packed` (possibly a peer's memory),
// from position 0 of the piece's packed stream, go into the layout laid at `mem`.
constexpr int kRowsMaxSegs = 64;
struct RowSeg {
    const void *packed;
    void *mem;
    size_t len;
};

struct RowsMultiPlan {
    int w;                                   // the slot width every kept piece moves with; 0: the row
                                             // kernel does not apply (nothing else below is valid)
    int nseg;                                // pieces kept
    int seg[kRowsMaxSegs];                   // their indices in the caller's list, in its order
    unsigned first_block[kRowsMaxSegs + 1];  // kept piece s owns blocks [first_block[s], first_block[s+1])
    size_t total;                            // bytes of the kept pieces
};

// the blocks of a plan's kept pieces (segs[p.seg[s]].len bytes each, p.total in all) at slot width w
template <class Seg>
inline void deal_row_blocks(RowsMultiPlan &p, const Seg *segs, int w, size_t per, size_t cap)
{
    unsigned next = 0;
    for (int s = 0; s < p.nseg; ++s) {
        p.first_block[s] = next;
        const size_t len = segs[p.seg[s]].len, nslots = len / (size_t)w;
        const size_t want = (nslots + per - 1) / per;
        const size_t share = (cap * len + p.total - 1) / p.total;
        size_t nb = want < share ? want : share;
        if (nb == 0) nb = 1;
        next += (unsigned)nb;
    }
    p.first_block[p.nseg] = next;
}

// Skips the pieces that hold no bytes and those whose packed source is their own memory base
// (nothing to move: k_multicopy's src == dst rule).  W is the widest power of two <= 16 that
// rows_width allows for EVERY kept piece -- its packed address, its memory address, its length,
// the stride and the extent -- so one odd piece lowers it for the whole launch.  Blocks are dealt
// as launch_multicopy deals them: a piece wants one block per `per` slots (per16 for W = 16, else
// per_narrow: lanes x slots per lane), gets at most its share by bytes of `cap` blocks (its blocks
// then loop), and at least one.
inline RowsMultiPlan plan_rows_multi(int64_t stride, int64_t extent, int64_t nblk, int64_t run_disp, int64_t run_len,
                                     const RowSeg *segs, int nseg, unsigned per16, unsigned per_narrow, size_t cap)
{
    RowsMultiPlan p;
    p.w = 0;
    p.nseg = 0;
    p.total = 0;
    p.first_block[0] = 0;
    if (nseg > kRowsMaxSegs || per16 == 0 || per_narrow == 0) return p;
    int w = 16;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].len == 0 || segs[i].packed == segs[i].mem) continue;
        const int wi = rows_width(stride, extent, nblk, 1, run_disp, run_len, segs[i].mem, segs[i].packed, 0,
                                  (int64_t)segs[i].len);
        if (wi == 0) return p;
        if (wi < w) w = wi;
        p.seg[p.nseg++] = i;
        p.total += segs[i].len;
    }
    deal_row_blocks(p, segs, w, w == 16 ? per16 : per_narrow, cap);
    p.w = w;
    return p;
}

// ---------------------------------------------------------------------------------------------
// One end of the two-ended row gather: a row layout of up to two levels -- rows of `run` bytes, the
// first at `disp`; level 0: nblk rows `stride` apart; level 1: n1 groups `step1` apart (n1 == 1: one
// level); instances `extent` apart; packed order instance, group, row, byte -- or dense bytes
// (nblk == 0: the piece is one row of its own length).  Also the record a sender publishes next to
// its counts (RankSlot::slay).
struct RowLay {
    int64_t nblk;  // 0: dense
    int64_t disp, run, stride, extent;
    int64_t n1 = 1, step1 = 0;  // no second level
};
inline RowLay row_dense() { return RowLay{0, 0, 0, 0, 0}; }

// The normal form: what a layout's tables hold (nruns runs at disp[] of len[] bytes per block, nblk
// blocks `stride` apart, instances `extent` apart) read as rows.  Returns the number of levels: 1
// rows, 2 rows in groups, 0 a run list (*out is then not meaningful).  The packed order of *out is the
// tables' order exactly.
//   * every run has one length > 0;
//   * the displacements are disp[0] + (r % p) * a + (r / p) * b for the smallest p dividing nruns;
//   * the levels, innermost first: (p, a), (nruns / p, b), (nblk, stride);
//   * a level of count 1 vanishes; an outer level whose step is the inner count times the inner step
//     merges into the inner one; a level 0 whose step is the run merges into the run;
//   * at most two levels may remain, and a layout of none is one row per instance.
// The two shapes that were rows before there were levels -- one run per block in the tables, and one
// block of equally spaced runs -- come out as they always did: {nblk, disp[0], len[0], stride, extent}
// and {nruns, disp[0], len[0], step, extent}, unmerged, so every launch made from them keeps its
// arguments.  max_levels 1 reads only those two shapes as rows (MI355X_KNOB_MOVE_ROW_LEVELS = 1).
inline int row_levels_view(const int64_t *disp, const int64_t *len, size_t nruns, int64_t nblk, int64_t stride,
                           int64_t extent, RowLay *out, int max_levels = 2)
{
    *out = RowLay{nblk, nruns ? disp[0] : 0, nruns ? len[0] : 0, stride, extent};
    if (nruns == 0 || len[0] <= 0) return 0;
    if (nruns == 1) return 1;
    for (size_t r = 1; r < nruns; ++r)
        if (len[r] != len[0]) return 0;
    size_t p = 0;
    int64_t a = 0, b = 0;
    for (size_t c = 1; c <= nruns && !p; ++c) {
        if (nruns % c) continue;
        a = c > 1 ? disp[1] - disp[0] : 0;
        b = c < nruns ? disp[c] - disp[0] : 0;
        bool ok = true;
        for (size_t r = 1; r < nruns && ok; ++r) ok = disp[r] == disp[0] + (int64_t)(r % c) * a + (int64_t)(r / c) * b;
        if (ok) p = c;
    }
    if (!p) return 0;
    if (nblk == 1 && (p == 1 || p == nruns)) {
        *out = RowLay{(int64_t)nruns, disp[0], len[0], disp[1] - disp[0], extent};
        return 1;
    }
    if (max_levels < 2) return 0;
    int64_t cnt[3] = {(int64_t)p, (int64_t)(nruns / p), nblk}, stp[3] = {a, b, stride};
    int n = 0;
    for (int i = 0; i < 3; ++i)
        if (cnt[i] != 1) {  // (a level of count 1 vanishes)
            cnt[n] = cnt[i];
            stp[n++] = stp[i];
        }
    for (int i = 0; i + 1 < n;) {
        if (stp[i + 1] != cnt[i] * stp[i]) {
            ++i;
            continue;
        }
        cnt[i] *= cnt[i + 1];
        for (int j = i + 1; j + 1 < n; ++j) cnt[j] = cnt[j + 1], stp[j] = stp[j + 1];
        --n;
    }
    int64_t run = len[0];
    while (n && stp[0] == run) {
        run *= cnt[0];
        for (int j = 0; j + 1 < n; ++j) cnt[j] = cnt[j + 1], stp[j] = stp[j + 1];
        --n;
    }
    if (n > 2) return 0;
    *out = RowLay{n ? cnt[0] : 1, disp[0], run, n ? stp[0] : 0, extent};
    if (n == 2) {
        out->n1 = cnt[1];
        out->step1 = stp[1];
    }
    return n == 2 ? 2 : 1;
}

// A send layout as the eligibility rule reads it (ddt.cpp fills it from a mi355x_ddt).
struct SendShape {
    int nruns;       // runs per block as the rule reads them: 1 when the layout is rows (row_levels_view)
    RowLay lay;      // the rows (meaningful when nruns == 1)
    int64_t size;    // packed bytes of one instance
    int levels() const { return nruns != 1 ? 0 : lay.n1 > 1 ? 2 : 1; }  // 0: a run list
};

// `most` instances leave no gap: the plain call (ddt_contiguous's rule)
inline bool send_gap_free(const SendShape &sh, size_t most)
{
    if (sh.nruns != 1) return false;
    if (sh.lay.nblk > 1 && sh.lay.stride != sh.lay.run) return false;
    if (sh.lay.n1 > 1 && sh.lay.step1 != sh.lay.nblk * sh.lay.run) return false;
    return most <= 1 || sh.lay.extent == sh.lay.n1 * sh.lay.nblk * sh.lay.run;
}

// May a sender publish this layout for its peers to pull from, instead of packing it?  All of:
// rows, of one level or two (a run list never); not gap-free for the call's largest count (that is the plain call); not in
// place; no byte below the buffer (run displacement, and either level's step and the extent >= 0
// wherever they count); every piece displacement >= 0 (displs may be NULL: none are given); every
// piece's packed size below kSlot32Max bytes and run length and both counts within 32 bits, so that a
// receiver can always serve the piece at slot width 1; the run at least min_run bytes, and min_run
// not 0 (never).
inline bool move_send_direct_ok(const SendShape &sh, const size_t *counts, const int64_t *displs, int n, bool in_place,
                                int64_t min_run)
{
    if (sh.nruns != 1 || in_place || min_run <= 0 || n < 0 || (n && !counts)) return false;
    const RowLay &l = sh.lay;
    if (l.run <= 0 || l.run < min_run || l.nblk < 1 || l.n1 < 1 || l.disp < 0) return false;
    size_t most = 0;
    for (int q = 0; q < n; ++q) most = counts[q] > most ? counts[q] : most;
    if (send_gap_free(sh, most)) return false;
    if ((l.nblk > 1 && l.stride < 0) || (l.n1 > 1 && l.step1 < 0) || (most > 1 && l.extent < 0)) return false;
    if (l.run >= ((int64_t)1 << 32) || l.nblk >= ((int64_t)1 << 32) || l.n1 >= ((int64_t)1 << 32)) return false;
    if (sh.size != l.n1 * l.nblk * l.run) return false;
    for (int q = 0; q < n; ++q) {
        if (displs && displs[q] < 0) return false;
        if (counts[q] >= (size_t)kSlot32Max / (size_t)sh.size + 1) return false;  // (no overflow in the product)
        if ((int64_t)counts[q] * sh.size >= kSlot32Max) return false;
    }
    return true;
}

// One end as the kernel holds it (the run's displacement is folded into the end's base pointer),
// and the byte offset of W-byte slot q of a piece's packed stream from that base: rows_pass' two
// divisions (one more with a second level), or q * W for a dense end.
struct RowEnd {
    int64_t stride, extent;
    FastDiv per_row, per_inst;  // slots per row, rows per group (per instance when there is one level)
    int64_t step1;
    FastDiv per_grp;            // groups per instance
};

inline RowEnd row_end(const RowLay &l, int w)
{
    RowEnd e;
    e.stride = l.nblk ? l.stride : 0;
    e.extent = l.nblk ? l.extent : 0;
    e.per_row = make_fastdiv(l.nblk ? (uint32_t)(l.run / w) : 1u);
    e.per_inst = make_fastdiv(l.nblk ? (uint32_t)l.nblk : 1u);
    e.step1 = l.nblk ? l.step1 : 0;
    e.per_grp = make_fastdiv(l.nblk ? (uint32_t)l.n1 : 1u);
    return e;
}

// the levels of an end: 0 dense, 1 rows, 2 rows in groups
inline int row_levels(const RowLay &l) { return l.nblk == 0 ? 0 : l.n1 > 1 ? 2 : 1; }

// LEVELS as row_levels gives them (a bool reads as before: false dense, true rows)
template <int W, int LEVELS> MI355X_HD int64_t row_slot_off(const RowEnd &e, uint32_t q)
{
    if constexpr (LEVELS == 0) return (int64_t)q * W;
    else {
        const uint32_t g = fast_div(q, e.per_row);
        const uint32_t w = q - g * e.per_row.d;
        const uint32_t h = fast_div(g, e.per_inst);
        const uint32_t i0 = g - h * e.per_inst.d;
        if constexpr (LEVELS == 1) return (int64_t)h * e.extent + (int64_t)i0 * e.stride + (int64_t)w * W;
        else {
            const uint32_t k = fast_div(h, e.per_grp);
            const uint32_t i1 = h - k * e.per_grp.d;
            return (int64_t)k * e.extent + (int64_t)i1 * e.step1 + (int64_t)i0 * e.stride + (int64_t)w * W;
        }
    }
}

// One launch of the two-ended gather.  Piece i: `len` bytes of a packed stream, read through the
// source layout `s` laid at `src` (possibly a peer's memory), written through the launch's one
// destination layout laid at `mem`; both from position 0 of the stream.
struct Row2Seg {
    const void *src;
    RowLay s;
    void *mem;
    size_t len;
};

// the widest width (16 .. 1) one end of a piece allows, 0: the 32-bit slot arithmetic does not hold it
inline int rows2_end_width(const RowLay &l, const void *base, size_t len)
{
    if (l.nblk == 0) {
        const uint64_t bits = (uintptr_t)base | (uint64_t)len;
        int w = 16;
        while (w > 1 && (bits & (uint64_t)(w - 1))) w >>= 1;
        return (int64_t)(len / (size_t)w) >= kSlot32Max ? 0 : w;
    }
    if (l.n1 < 1 || l.n1 >= ((int64_t)1 << 32)) return 0;
    // (rows_width only folds the extent into the bits that bound W: the second step joins them there)
    return rows_width(l.stride, (int64_t)((uint64_t)l.extent | (uint64_t)l.step1), l.nblk, 1, l.disp, l.run, base, nullptr, 0,
                      (int64_t)len);
}

// plan_rows_multi's contract with two ends.  Kept: the pieces that hold bytes (in the caller's
// order); p.seg / p.nseg / p.total as there.  W is the widest power of two <= 16 that EVERY kept
// piece allows on BOTH ends: for a row end its first byte (base + disp), run length, stride, second
// step and extent, for a dense end (one row) its base; and the piece length.  An end beyond the 32-bit
// slot arithmetic (rows_width's limits, and the group count below 2^32; a dense end: kSlot32Max
// slots) makes the plan decline (w = 0).
// Blocks are dealt exactly as plan_rows_multi deals them.
inline RowsMultiPlan plan_rows2_multi(const RowLay &dst, const Row2Seg *segs, int nseg, unsigned per16, unsigned per_narrow,
                                      size_t cap)
{
    RowsMultiPlan p;
    p.w = 0;
    p.nseg = 0;
    p.total = 0;
    p.first_block[0] = 0;
    if (nseg > kRowsMaxSegs || per16 == 0 || per_narrow == 0) return p;
    int w = 16;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].len == 0) continue;
        const int ws = rows2_end_width(segs[i].s, segs[i].src, segs[i].len);
        const int wd = rows2_end_width(dst, segs[i].mem, segs[i].len);
        if (ws == 0 || wd == 0) return p;
        if (ws < w) w = ws;
        if (wd < w) w = wd;
        p.seg[p.nseg++] = i;
        p.total += segs[i].len;
    }
    // each end was checked at its own width; the shared W may be narrower, so the counts larger
    for (int s = 0; s < p.nseg; ++s) {
        const Row2Seg &g = segs[p.seg[s]];
        const int64_t rs = g.s.nblk ? g.s.run / w : 0, rd = dst.nblk ? dst.run / w : 0;
        if ((int64_t)(g.len / (size_t)w) >= kSlot32Max || rs >= ((int64_t)1 << 32) || rd >= ((int64_t)1 << 32)) {
            p.nseg = 0;
            p.total = 0;
            return p;
        }
    }
    deal_row_blocks(p, segs, w, w == 16 ? per16 : per_narrow, cap);
    p.w = w;
    return p;
}

} // namespace mi355x
