// ddt_rows_plan.hpp -- the host side of the row kernels' launches (ddt_kernels.hip), plain C++ so
// tools/rows_plan_check.cpp compiles it for the host alone:
//   * rows_width: the slot width one window of a row layout (one run per block) can move with;
//   * plan_rows_multi: one launch unpacking several packed pieces into the same row layout (the pull
//     of a movement collective into a derived receive datatype): which pieces it keeps, the slot
//     width they share and the blocks each one gets.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mi355x {

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
    const size_t per = w == 16 ? per16 : per_narrow;
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
    p.w = w;
    return p;
}

} // namespace mi355x
