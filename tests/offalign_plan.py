"""Case tables of the multi-process off-alignment run (ipc_worker.py::offalign), and the address
tests of the device code restated in Python so that test_offalign_plan.py can show, without a GPU,
which branch every case enters.  Pure Python: no numpy, no torch.

Shifts are bytes past a 16-byte boundary (devbuf.Buf's `shift`); every shift is a multiple of the
element type's C alignment.  A slot is (op, type, element size, alignment, shift pairs); a pair is
(sbuf shift, rbuf shift)."""
from __future__ import annotations

LL_SLICE = 4096      # kLLChunk, coll_internal.hpp:100: payload bytes per workgroup, 16 per thread
SVC_PASS = 4         # kSvcPass, coll_svc.hip:40
LL_MAX_RANKS = 8     # kLLMaxRanks, coll_internal.hpp:101: the LL and service forms stop here
FOLD_CHUNK = 8       # kFoldChunk, coll_internal.hpp:12

SLOTS = [
    ("BXOR", "INT8", 1, 1, [(1, 1), (1, 2), (3, 0), (0, 5)]),
    ("SUM", "INT16", 2, 2, [(2, 2), (6, 10), (4, 4), (0, 2)]),
    ("SUM", "FLOAT", 4, 4, [(4, 4), (4, 8), (12, 0), (0, 4)]),
    ("MINLOC", "FLOAT_INT", 8, 4, [(4, 4), (4, 12), (8, 0)]),
    ("MAX", "DOUBLE", 8, 8, [(8, 8), (8, 0), (0, 8)]),
    ("PROD", "C_DOUBLE_COMPLEX", 16, 8, [(8, 8), (8, 0), (0, 8)]),
    ("MAXLOC", "DOUBLE_INT", 16, 8, [(8, 8), (8, 0), (0, 8)]),
]
ARRANGEMENTS = ("same", "rotated")
CONTROL = None       # pair index of the (0, 0) control, run once per slot

AR_ALGS = (0, 3, 4)  # ALLREDUCE_ALG: the decision, recursive doubling, ring


def slot(op: str, ty: str):
    return next(s for s in SLOTS if s[0] == op and s[1] == ty)


def ll_cases(pairs, arrangements=ARRANGEMENTS):
    """(pair index, arrangement) of one slot: the control once, then every pair in every arrangement"""
    return [(CONTROL, "same")] + [(i, a) for i in range(len(pairs)) for a in arrangements]


def shifts(pairs, i, arrangement: str, rank: int):
    """rank's (sbuf shift, rbuf shift): same -- pair i on every rank; rotated -- pair (i + rank) mod len"""
    if i is CONTROL:
        return (0, 0)
    return pairs[i] if arrangement == "same" else pairs[(i + rank) % len(pairs)]


def payload_sizes(esz: int, limit: int):
    """bytes, rounded down to whole elements: one element, one element short of a slice, one past it
    (a second slice of thread 0), more than SVC_PASS slices with a last thread of len < 16, the limit"""
    raw = [esz, LL_SLICE - esz, LL_SLICE + esz, (SVC_PASS + 1) * LL_SLICE + 16 + esz, limit]
    return [b // esz * esz for b in raw]


def roots(size: int):
    return (0, size - 1)


# ---------------------------------------------------------------- parts (a) and (b): the LL forms
LL_COPY_SHIFTS = [(0, 0), (1, 2), (4, 8), (3, 3)]   # (src, dst) of allgather / bcast


def ll_copy_sizes(limit: int):
    return [1, 13, 4097, limit]


def ll_reduction_calls(size: int, limit: int, algs=AR_ALGS, arrangements=ARRANGEMENTS, reduce_too=True) -> int:
    """calls of the allreduce / reduce table: per (slot, pair, arrangement, size) every algorithm in
    place and not, and a reduce to each root"""
    per_case = 2 * len(algs) + (len(roots(size)) if reduce_too else 0)
    return sum(len(ll_cases(s[4], arrangements)) * len(payload_sizes(s[2], limit)) * per_case for s in SLOTS)


def ll_copy_calls(size: int, limit: int) -> int:
    """allgather not in place and in place, bcast from each root, per (size, shifts)"""
    return len(ll_copy_sizes(limit)) * len(LL_COPY_SHIFTS) * (2 + len(roots(size)))


# ---------------------------------------------------------------- part (c): pull allreduce
PULL_SLOTS = [("SUM", "FLOAT"), ("MAX", "DOUBLE"), ("PROD", "C_DOUBLE_COMPLEX")]
PULL_BACK_TO_BACK = 64


def pull_counts(svc_max: int, esz: int):
    return [svc_max // esz + 1, 100_003 // esz]


def pull_calls(svc_max: int):
    """(served, refused) of part (c): per (slot, count) steps 1 and 4 are served, 2 and 3 refused"""
    n = sum(len(pull_counts(svc_max, slot(*s)[2])) for s in PULL_SLOTS)
    return 2 * n, 2 * n


# ---------------------------------------------------------------- part (d): pull copies, reduce_scatter
PULL_COPY_SHIFTS = [(0, 0), (4, 8), (1, 2), (0, 4)]
RS_SLOTS = [("SUM", "FLOAT"), ("BXOR", "INT8"), ("SUM", "INT16"), ("MAXLOC", "DOUBLE_INT")]
RS_ALGS = (0, 3)


def pull_copy_sizes(svc_max: int):
    return [svc_max + 16, svc_max + 1, 100_003]


def pull_copy_calls(size: int, svc_max: int) -> int:
    return len(pull_copy_sizes(svc_max)) * len(PULL_COPY_SHIFTS) * (2 + len(roots(size)))


def rs_counts(size: int, limit: int, esz: int):
    return [[7 * r + 3 for r in range(size)], [limit // esz - r for r in range(size)]]


def rs_calls() -> int:
    return len(RS_SLOTS) * 2 * 2 * len(RS_ALGS)   # (counts, first two pairs, algorithms)


# ---------------------------------------------------------------- part (e): pipelined allreduce
PIPE_SLOTS = [("SUM", "FLOAT", 4, 4), ("PROD", "C_DOUBLE_COMPLEX", 16, 8), ("MAXLOC", "DOUBLE_INT", 16, 8),
              ("BAND", "INT64", 8, 8)]
PIPE_CHUNK_KIB = 1   # the smallest chunk the knob sets (0 selects the automatic size, coll_pipe_host.cpp:100)


def pipe_chunk_elems(esz: int) -> int:
    """coll_pipe_host.cpp:99-104 for blocks far below kPipeKmax chunks: whole 16-byte vectors"""
    vec = 16 // esz
    return ((PIPE_CHUNK_KIB << 10) // esz + vec - 1) // vec * vec


def pipe_count(size: int, esz: int) -> int:
    """three chunks per block, the last one short, blocks of unequal length"""
    return size * (5 * pipe_chunk_elems(esz) // 2) + size + 3


def pipe_layouts(esz: int, align: int):
    """aligned; one non-zero shift on every buffer (the alignment, then 16 - esz where that is
    another non-zero shift); rotated; only the rbufs of odd ranks shifted"""
    same = [align] + ([16 - esz] if 16 - esz not in (0, align) else [])
    return ["aligned"] + [f"same{m}" for m in same] + ["rotated", "odd"]


def pipe_shifts(layout: str, align: int, rank: int):
    """rank's (sbuf shift, rbuf shift); in place the one buffer takes the rbuf shift"""
    if layout == "aligned":
        return (0, 0)
    if layout.startswith("same"):
        return (int(layout[4:]),) * 2
    if layout == "rotated":   # the multiples of the alignment below 16, one step apart for sbuf and rbuf
        steps = list(range(0, 16, align))
        return steps[rank % len(steps)], steps[(rank + 1) % len(steps)]
    assert layout == "odd"
    return 0, (align if rank & 1 else 0)


def pipe_calls() -> int:
    """pipelined calls: per (slot, layout) PIPE_WT 0 and 1, in place and not"""
    return sum(len(pipe_layouts(s[2], s[3])) * 4 for s in PIPE_SLOTS)


def pipe_two_phase_calls() -> int:
    """the same inputs once with PIPE = 0: per (slot, layout) in place and not"""
    return sum(len(pipe_layouts(s[2], s[3])) * 2 for s in PIPE_SLOTS)


# ---------------------------------------------------------------- the device code's address tests
def ll_read16_sys(addr16: int, length: int) -> str:
    """coll_ll_dev.hpp:47-61, ll_read16<SYS>: one 16-byte buffer load, whole words, single bytes"""
    if length == 16 and addr16 % 16 == 0:
        return "vec"
    return "word" if addr16 % 4 == 0 and length % 4 == 0 else "byte"


def ll_write16_sys(addr16: int, length: int) -> str:
    """coll_ll_dev.hpp:81-97, ll_write16<SYS>: the same three forms for the store"""
    if length == 16 and addr16 % 16 == 0:
        return "vec"
    return "word" if addr16 % 4 == 0 and length % 4 == 0 else "byte"


def ll_pieces(nbytes: int):
    """(byte offset, len) of every thread's piece of a call, coll_ll_dev.hpp:119-128 (ll_block);
    offsets are multiples of 16, so a piece's address mod 16 is the buffer's"""
    return [(off, min(16, nbytes - off)) for off in range(0, nbytes, 16)]


def svc_copy_seg(src16: int, dst16: int, length: int) -> str:
    """coll_svc.hip:130-155: 16-byte vectors, words or bytes for the whole segment, by both ends
    and the length together"""
    if (src16 | dst16 | length) % 16 == 0:
        return "vec"
    return "word" if (src16 | dst16 | length) % 4 == 0 else "byte"


def co_aligned(esz: int, addrs16) -> bool:
    """stream_core.hpp:49-55: every pointer shares the first one's misalignment, a whole element"""
    m = addrs16[0] % 16
    return m % esz == 0 and all(a % 16 == m for a in addrs16)


def split16(n: int, esz: int, m: int, co: bool):
    """stream_core.hpp:37-46 as (head, 16-byte vectors, tail) in elements; operands that are not
    co-aligned take the whole range element-wise"""
    if not (co and m % esz == 0):
        return n, 0, 0
    head = min((16 - m) // esz if m else 0, n)
    nvec = (n - head) // (16 // esz)
    return head, nvec, n - head - nvec * (16 // esz)


def split16_form(n: int, esz: int, m: int, co: bool) -> str:
    head, nvec, tail = split16(n, esz, m, co)
    if nvec == 0:
        return "scalar"
    return "/".join(p for p, k in (("head", head), ("body", nvec), ("tail", tail)) if k)


def ring_block(count: int, n: int, b: int):
    """coll_sched.cpp:365-371 (the reference's COLL_TUNED_COMPUTE_BLOCKCOUNT): (offset, length)"""
    late, split = divmod(count, n)
    early = late + 1 if split else late
    return (b * early, early) if b < split else (b * late + split, late)


def pipe_case(size: int, esz: int, me: int, sshift, rshift, inplace: bool, wt: int):
    """what k_pipe_allreduce does on rank `me` (coll_pipe_host.cpp:132-138, coll_pipe.hip:80-100,
    :162-166, :181-184): co_fold and the shared misalignment m, the co_pull mask, and per chunk of
    my block the fold's split and whether it is stored write-through"""
    count, chunk = pipe_count(size, esz), pipe_chunk_elems(esz)
    dst = [rshift[q] for q in range(size)]
    src = [dst[q] if inplace else sshift[q] for q in range(size)]
    co_fold = co_aligned(esz, [dst[me]] + src)
    co_pull = sum(1 << q for q in range(size) if dst[q] % 16 == dst[me] % 16)
    boff, blen = ring_block(count, size, me)
    chunks = []
    for lo in range(0, blen, chunk):
        hi = min(lo + chunk, blen)
        a16 = (dst[me] + (boff + lo) * esz) % 16
        chunks.append({"form": split16_form(hi - lo, esz, a16 & (16 - esz), co_fold),
                       "wt": bool(wt and co_fold and a16 == 0 and (hi - lo) * esz % 16 == 0)})
    return {"co_fold": co_fold, "m": dst[me] % 16, "co_pull": co_pull, "all": (1 << size) - 1, "chunks": chunks,
            "load_groups": -(-size // FOLD_CHUNK) if size > 4 else 1, "blen": blen}
