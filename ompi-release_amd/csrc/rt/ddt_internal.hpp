// ddt_internal.hpp -- device view of a datatype layout (see ddt_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddt_rows_plan.hpp"

struct mi355x_ddt;

namespace mi355x {

// true when `count` instances occupy one gap-free byte range starting at base + *first (ddt.cpp)
bool ddt_contiguous(const mi355x_ddt *d, size_t count, int64_t *first);

struct DdtDev {
    const int64_t *disp;   // run displacement inside a block (device array)
    const int64_t *len;    // run length in bytes
    const int64_t *pfx;    // packed offset of the run inside a block
    const int64_t *pfx_host;  // the packed offsets and lengths in host memory
    const int64_t *len_host;
    int nruns;
    int64_t nblk, stride, extent;
    int64_t blk_bytes, inst_bytes;
    uint64_t run_bits;     // OR of every run's displacement and length (their common alignment)
    int64_t max_len;       // longest run
};

// launch shape of the row kernel: slots per lane (2, 4, 8) and the non-temporal mask
// (-1 auto: kDdtAutoNT above 256 MiB of traffic; else 1 = loads, 2 = stores)
constexpr int kDdtAutoNT = 3;
struct DdtTune {
    int unroll_pack = 4;
    int unroll_unpack = 2;
    int threads = 256;
    int nontemporal = -1;
    // mi355x_ddt_tune_rows: 2 row kernel any slot width + unit kernel (16-B packed slots over 8/4-B
    // aligned runs where the packed side allows), 3 the same with W-byte units only, 1 16-B rows
    // only, 0 neither
    int rows = 2;
};
DdtTune &ddt_tune();

// csum: NULL, or where the window's checksum goes (the launch is then waited for)
int launch_ddt(const DdtDev &d, bool pack, void *mem, void *packed, int64_t pos, int64_t bytes, unsigned *csum,
               hipStream_t s);
// the row kernel (one run per block, slots of the widest power-of-two width <= 16 B every
// address and length allows); returns 1 when it does not apply
int launch_ddt_rows(const DdtDev &d, int nruns_host, int64_t run_disp, int64_t run_len, bool pack, void *mem,
                    void *packed, int64_t pos, int64_t bytes, unsigned *csum, hipStream_t s);
// the row kernel's unpack of several packed pieces (each from position 0 of its own stream) into the
// same one-run layout in one launch (plan_rows_multi, ddt_rows_plan.hpp); returns 1 when it does
// not apply
int launch_ddt_rows_multi(const DdtDev &d, int64_t run_disp, int64_t run_len, const RowSeg *segs, int nseg,
                          hipStream_t s);
// the pull of a movement collective into a receive layout (coll_move.cpp): piece i = len[i] packed
// bytes at src[i], which may be a peer's mapped memory, unpacked into d laid at mem[i].  A row
// layout takes one launch: k_ddt_rows_multi when its tables hold one run per block, else -- rows of
// up to two levels in the normal form (row_levels_view), and a piece table given (the caller gives
// none under MI355X_KNOB_MOVE_ROW_LEVELS = 1) -- the two-ended row gather with dense sources.  Any
// other goes piece by piece through launch_ddt.  *launches (may be NULL) grows by the kernels
// launched.  Nothing is waited for.
struct Rows2Table;
int ddt_unpack_segments(const mi355x_ddt *d, const void *const *src, void *const *mem, const size_t *len, int nseg,
                        hipStream_t s, const Rows2Table *tab = nullptr, uint64_t *launches = nullptr);

// the eligibility rule's view of a layout (ddt_rows_plan.hpp: move_send_direct_ok); max_levels 1
// reads as rows only what was rows before there were levels (row_levels_view)
SendShape ddt_send_shape(const mi355x_ddt *d, int max_levels = 2);
// the two-ended row gather's per-piece table: device memory the kernel reads, and the pinned host
// copy it is filled in (both kRows2TableBytes; the communicator owns them, coll_move.cpp)
constexpr size_t kRows2TableBytes = 96 * (size_t)kRowsMaxSegs;
struct Rows2Table {
    void *dev, *host;
};
// one launch: piece i read through its own source layout, written through dst (ddt_kernels.hip);
// returns 1 when the plan declines (plan_rows2_multi: an end beyond the 32-bit slot arithmetic)
int launch_ddt_rows2_multi(const RowLay &dst, const Row2Seg *segs, int nseg, const Rows2Table &tab, hipStream_t s);
// the pull of a movement collective out of published send layouts: piece i = segs[i].len bytes read
// through segs[i].s at segs[i].src, written through d laid at segs[i].mem (d NULL: dense bytes).  One
// launch; returns 1 when it does not apply -- d is a run list (or rows that max_levels keeps off the
// launch), or the plan declines -- and the caller gathers into dense scratch first.
// mi355x_ddt_tune_rows is not consulted: a receiver serves whatever a sender was allowed to publish.
// *launches as above.  Nothing is waited for.
int ddt_gather_segments(const mi355x_ddt *d, const Row2Seg *segs, int nseg, const Rows2Table &tab, hipStream_t s,
                        int max_levels = 2, uint64_t *launches = nullptr);

} // namespace mi355x
