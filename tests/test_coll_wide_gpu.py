"""The kernels of coll_kernels.hip past their first load chunk, on every slot, off alignment.

k_fold, k_ring_all and k_scan_part load ranks in chunks of kFoldChunk = 8 and loop over further
chunks, k_tree runs a 16-register program (kTreeMax) and the fold's role mask is 64 bits wide; the
other loopback suites stop at 8 ranks (the scans at 9).  Here the same calls run on loopback
communicators of 9, 10, 16, 17 and 33 ranks (a second chunk of one rank, the first held-back store
of the exclusive scan, a full tree, the first size without a tree and with a third chunk, a fifth
chunk and role bit 32), every slot of the four families runs once, and the launchers' alignment
branches (head peel, `m % sizeof(T) != 0`, element-wise) are entered with guard bytes around every
result buffer.

Loopback never takes the LL, service or pipelined paths, so the knobs named in
each docstring select the kernel family by the conditions of allreduce_impl, reduce_impl,
nbc_allreduce_impl and scan_part.  Expected bits: the oracle's simulation of the reference
schedules (tests/nbc_oracle.py and tests/nbc_scan_oracle.py under NB_ORDER = 1).  Bar:
opdata.assert_same, the suite's bit-exact comparison with its two documented relaxations.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import nbc_oracle as nbc
import opdata
import test_nbc_gpu as tnbc
import test_scan_part_gpu as tscan
from devbuf import GUARD, Buf, knobs  # noqa: F401  (shared with ipc_worker.py::offalign)
from test_coll_gpu import CASES, _ptrs, run_ranks

pytestmark = pytest.mark.gpu

ONE_PHASE = 1 << 20  # the communicators' default ONE_PHASE_MAX_BYTES
UNSUPPORTED = -2    # MI355X_ERR_UNSUPPORTED
RING_SLOTS = [("SUM", "FLOAT"), ("PROD", "C_DOUBLE_COMPLEX"), ("MAXLOC", "DOUBLE_INT")]   # test_one_phase_ring's


@pytest.fixture(scope="module")
def comms(gpu, pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.Comm.loopback(n, 0)
            for c in made[n]:
                c.set("TIMEOUT_S", 60)
        return made[n]

    yield get
    for cs in made.values():
        for c in cs:
            c.destroy()


def run_calls(torch, cs, calls):
    """calls: functions of the rank, run in order by one thread per rank; returns rank 0's
    last_algorithm() after each"""
    algs = [None] * len(calls)
    torch.cuda.synchronize()

    def rank(r):
        torch.cuda.set_device(0)
        for i, call in enumerate(calls):
            call(r)
            if r == 0:
                algs[i] = cs[0].last_algorithm()

    run_ranks(len(cs), rank)
    torch.cuda.synchronize()
    return algs


def _allreduce_case(torch, pkg, oracle, cs, alg, slot, count, inplace, salt, one_phase=None, sshift=None, rshift=None):
    """one allreduce call: (post(rank), check(last_algorithm)); the knob ONE_PHASE_MAX_BYTES is set
    per call by every rank when `one_phase` is given; sshift / rshift: per-rank byte offsets"""
    n = len(cs)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    xs = [opdata.make(tname, count, salt + r) for r in range(n)]
    outs = [np.zeros_like(xs[0]) for _ in range(n)]
    ran = oracle.oracle_allreduce(alg, n, count, ty, op, 0, _ptrs(xs), _ptrs(outs))
    assert ran >= 0
    sshift, rshift = sshift or [0] * n, rshift or [0] * n
    dx = [Buf(torch, xs[r], count, sshift[r], xs[r]) for r in range(n)]
    dr = dx if inplace else [Buf(torch, xs[r], count, rshift[r]) for r in range(n)]

    def post(r):
        if one_phase is not None:
            cs[r].set("ONE_PHASE_MAX_BYTES", one_phase)
        cs[r].allreduce(None if inplace else dx[r].ptr, dr[r].ptr, count, ty, op)

    def check(got_alg):
        what = f"allreduce n={n} alg={alg} count={count} inplace={inplace} one_phase={one_phase}"
        assert got_alg == ran, what
        got = [dr[r].get() for r in range(n)]
        for r in range(n):
            opdata.assert_same(tname, opname, got[r], outs[r], f"{what} rank={r}")
            assert dr[r].guards_intact(), f"{what} rank={r}: wrote outside rbuf"
        return got

    return post, check


def _run_cases(torch, cs, cases):
    algs = run_calls(torch, cs, [post for post, _ in cases])
    return [check(a) for (_, check), a in zip(cases, algs)]


# ------------------------------------------------------------------ 1. k_fold beyond one chunk
@pytest.mark.parametrize("n,push", [(9, 0), (17, 0), (33, 0), (9, 1), (17, 1)])
@pytest.mark.parametrize("inplace", [False, True])
def test_fold_allreduce(gpu, pkg, oracle, comms, n, push, inplace):
    """ALLREDUCE_ALG 4 with ONE_PHASE_MAX_BYTES 0: owner-computes, rank r folds ring block r of the
    n inputs in one k_fold launch (2, 3 and 5 load chunks) and pulls the rest (k_multicopy); with
    PUSH 1 the fold writes its block into all n rbufs (nd = n).  Counts n, 4n + 3 and 67n + 5: one
    element per block, scalar blocks, blocks with a head, a 16-byte body and a tail."""
    cs = comms(n)
    with knobs(cs, ALLREDUCE_ALG=4, ONE_PHASE_MAX_BYTES=0, PUSH=push):
        cases = [_allreduce_case(gpu, pkg, oracle, cs, 4, slot, count, inplace, 100 + 40 * i)
                 for i, slot in enumerate(CASES) for count in (n, 4 * n + 3, 67 * n + 5)]
        _run_cases(gpu, cs, cases)


@pytest.mark.parametrize("n", [9, 17, 33])
@pytest.mark.parametrize("alg", [1, 3])
def test_fold_reduce(gpu, pkg, oracle, comms, n, alg):
    """REDUCE_ALG 1 (linear) and 3 (pipeline): every step keeps the accumulator as `out`, so every
    bit of the 64-bit role mask up to n - 1 is set -- MAX/DOUBLE and MAXLOC/FLOAT_INT see a wrong
    role bit, fp32 SUM a wrong order.  ONE_PHASE_MAX_BYTES 1 << 20: the root folds the whole vector
    in one k_fold launch; 0: every rank folds its ring block (the root into rbuf, the others into
    scratch) and the root pulls.  Roots 0 and n - 1, in place at the root and not."""
    torch, cs = gpu, comms(n)
    cases = []
    for i, (opname, tname) in enumerate(CASES[:6]):
        op, ty = pkg.OP[opname], pkg.T[tname]
        for count, one_phase in ((4 * n + 3, ONE_PHASE), (67 * n + 5, ONE_PHASE), (67 * n + 5, 0)):
            xs = [opdata.make(tname, count, 800 + 40 * i + r) for r in range(n)]
            for root in (0, n - 1):
                want = np.zeros_like(xs[0])
                assert oracle.oracle_reduce(alg, n, root, count, ty, op, 0, _ptrs(xs), want.ctypes.data) == alg
                for inplace in (False, True):
                    cases.append(_reduce_case(torch, pkg, cs, slot=(opname, tname), xs=xs, want=want, root=root,
                                              inplace=inplace, one_phase=one_phase, alg=alg))
    with knobs(cs, REDUCE_ALG=alg, ONE_PHASE_MAX_BYTES=ONE_PHASE):
        _run_cases(torch, cs, cases)


def _reduce_case(torch, pkg, cs, slot, xs, want, root, inplace, one_phase, alg):
    n, count = len(xs), len(xs[0])
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    dx = [Buf(torch, xs[r], count, 0, xs[r]) for r in range(n)]
    dr = dx[root] if inplace else Buf(torch, xs[0], count)

    def post(r):
        cs[r].set("ONE_PHASE_MAX_BYTES", one_phase)
        cs[r].reduce(None if (inplace and r == root) else dx[r].ptr, dr.ptr if r == root else None, count, ty, op, root)

    def check(got_alg):
        what = f"reduce n={n} alg={alg} root={root} count={count} inplace={inplace} one_phase={one_phase}"
        assert got_alg == alg, what
        opdata.assert_same(tname, opname, dr.get(), want, what)
        assert dr.guards_intact(), f"{what}: wrote outside rbuf"

    return post, check


def _pipeline_rcount(oracle, n, ty, esz):
    """a block length at which the fixed reduce decision takes the pipeline (a fold) for n ranks"""
    for target in (28_000, 200_000):
        rcount = target // (n * esz) + 1
        if oracle.oracle_reduce_decision(n, rcount * n, ty, None) == 3:
            return rcount
    raise AssertionError(f"no pipeline region found for n={n}")


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("inplace", [False, True])
def test_fold_reduce_scatter_block(gpu, pkg, oracle, comms, n, inplace):
    """MPI_Reduce_scatter_block is a reduce to rank 0 + scatter: rank r folds block r with the reduce
    program.  Blocks of 1 and 37 elements under REDUCE_ALG 3 (the fixed decision takes a tree at
    these sizes, which 17 ranks do not have), and a block in the decision's own pipeline region
    (oracle_reduce_decision == 3) with no algorithm forced -- each a k_fold launch over n inputs."""
    torch, cs = gpu, comms(n)
    cases = []
    for i, (opname, tname) in enumerate(CASES):
        op, ty = pkg.OP[opname], pkg.T[tname]
        esz = pkg.type_size(ty)
        for rcount, forced in ((1, 3), (37, 3), (_pipeline_rcount(oracle, n, ty, esz), 0)):
            total = rcount * n
            xs = [opdata.make(tname, total, 200 + 40 * i + r) for r in range(n)]
            outs = [np.zeros(rcount, dtype=xs[0].dtype) for _ in range(n)]
            if forced:
                whole = np.zeros_like(xs[0])
                assert oracle.oracle_reduce(forced, n, 0, total, ty, op, 0, _ptrs(xs), whole.ctypes.data) == forced
                outs = [whole[r * rcount:(r + 1) * rcount].copy() for r in range(n)]
            else:
                assert oracle.oracle_reduce_scatter_block(n, rcount, ty, op, _ptrs(xs), _ptrs(outs)) == 3
            dx = [Buf(torch, xs[r], total, 0, xs[r]) for r in range(n)]
            dr = dx if inplace else [Buf(torch, xs[r], rcount) for r in range(n)]

            def post(r, dx=dx, dr=dr, rcount=rcount, forced=forced, ty=ty, op=op):
                cs[r].set("REDUCE_ALG", forced)
                cs[r].reduce_scatter_block(None if inplace else dx[r].ptr, dr[r].ptr, rcount, ty, op)

            def check(got_alg, dr=dr, outs=outs, rcount=rcount, opname=opname, tname=tname):
                assert got_alg == 3
                for r in range(n):
                    what = f"rsb n={n} rcount={rcount} inplace={inplace} rank={r}"
                    opdata.assert_same(tname, opname, dr[r].get(rcount), outs[r], what)
                    assert dr[r].guards_intact(), f"{what}: wrote outside rbuf"

            cases.append((post, check))
    with knobs(cs, REDUCE_ALG=0):
        _run_cases(torch, cs, cases)


@pytest.mark.parametrize("n", [9, 17])
def test_fold_reduce_scatter_ring(gpu, pkg, oracle, comms, n):
    """REDUCE_SCATTER_ALG 3: rank r folds its block in the ring's order (k_fold over n inputs, the
    accumulator as `in`); the counts include zeros, at both ends of the communicator too"""
    torch, cs = gpu, comms(n)
    oracle.oracle_reduce_scatter_alg.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                 ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p)]
    small = [(5 * r + 2) % 4 for r in range(n)]
    large = [67 + 3 * (r % 4) for r in range(n)]
    large[0] = large[n // 2] = large[n - 1] = 0
    assert 0 in small
    cases = []
    for i, (opname, tname) in enumerate(CASES):
        op, ty = pkg.OP[opname], pkg.T[tname]
        for rcounts in (small, large):
            total = sum(rcounts)
            xs = [opdata.make(tname, total, 300 + 40 * i + r) for r in range(n)]
            outs = [np.zeros(max(k, 1), dtype=xs[0].dtype) for k in rcounts]
            rc = (ctypes.c_int * n)(*rcounts)
            assert oracle.oracle_reduce_scatter_alg(3, n, rc, ty, op, _ptrs(xs), _ptrs(outs)) == 3
            dx = [Buf(torch, xs[r], total, 0, xs[r]) for r in range(n)]
            dr = [Buf(torch, xs[r], max(k, 1)) for r, k in enumerate(rcounts)]

            def post(r, dx=dx, dr=dr, rcounts=rcounts, ty=ty, op=op):
                cs[r].reduce_scatter(dx[r].ptr, dr[r].ptr, rcounts, ty, op)

            def check(got_alg, dr=dr, outs=outs, rcounts=rcounts, opname=opname, tname=tname):
                assert got_alg == 3
                for r in range(n):
                    what = f"rs ring n={n} rank={r} rcounts={rcounts}"
                    if rcounts[r]:
                        opdata.assert_same(tname, opname, dr[r].get(rcounts[r]), outs[r][:rcounts[r]], what)
                    else:
                        assert dr[r].holds(None), f"{what}: a rank that receives nothing was written"
                    assert dr[r].guards_intact(), f"{what}: wrote outside rbuf"

            cases.append((post, check))
    with knobs(cs, REDUCE_SCATTER_ALG=3):
        _run_cases(torch, cs, cases)


# ------------------------------------------------------------------ 2. k_tree past register 8
@pytest.mark.parametrize("n,alg", [(9, 3), (11, 3), (16, 3), (9, 1), (9, 2)])
def test_tree_allreduce(gpu, pkg, oracle, comms, n, alg):
    """ALLREDUCE_ALG 3 (recursive doubling), not in place: every rank evaluates the whole vector in
    one k_tree launch over n registers -- 9 and 11 with the non-power-of-two pre-step, 16 the full
    register file.  Algorithms 1 (linear: a fold) and 2 (nonoverlapping: the reduce decision's tree
    to rank 0) at n = 9 through the same branch of allreduce_impl."""
    cs = comms(n)
    with knobs(cs, ALLREDUCE_ALG=alg):
        cases = [_allreduce_case(gpu, pkg, oracle, cs, alg, slot, count, False, 1100 + 40 * i)
                 for i, slot in enumerate(CASES) for count in (7, 67 * n + 5)]
        _run_cases(gpu, cs, cases)


@pytest.mark.parametrize("n", [9, 13, 16])
@pytest.mark.parametrize("alg", [2, 4, 5])
def test_tree_reduce(gpu, pkg, oracle, comms, n, alg):
    """REDUCE_ALG 2 (chain, default fan-out 4), 4 (binary) and 5 (binomial): k_tree programs over up
    to 16 registers, roots 0 and n - 1.  ONE_PHASE_MAX_BYTES 1 << 20: the root evaluates the vector
    (in place and not); 0: every rank evaluates its ring block and the root pulls."""
    torch, cs = gpu, comms(n)
    cases = []
    for i, (opname, tname) in enumerate(CASES[:6]):
        op, ty = pkg.OP[opname], pkg.T[tname]
        for count, one_phase, inplace in ((7, ONE_PHASE, False), (67 * n + 5, ONE_PHASE, True), (67 * n + 5, 0, False)):
            xs = [opdata.make(tname, count, 1300 + 40 * i + r) for r in range(n)]
            for root in (0, n - 1):
                want = np.zeros_like(xs[0])
                assert oracle.oracle_reduce(alg, n, root, count, ty, op, 0, _ptrs(xs), want.ctypes.data) == alg
                cases.append(_reduce_case(torch, pkg, cs, slot=(opname, tname), xs=xs, want=want, root=root,
                                          inplace=inplace, one_phase=one_phase, alg=alg))
    with knobs(cs, REDUCE_ALG=alg, ONE_PHASE_MAX_BYTES=ONE_PHASE):
        _run_cases(torch, cs, cases)


@pytest.mark.parametrize("slot", tnbc.SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", [9, 16])
def test_tree_libnbc(gpu, pkg, oracle, comms, n, slot):
    """NB_ORDER 1, below libnbc's 64 KiB threshold: MPI_Iallreduce and MPI_Ireduce run libnbc's
    binomial tree, a `three` program in k_tree (MAXLOC / MINLOC: the THREE instantiation) over 9 and
    16 registers.  Not in place and <= ONE_PHASE_MAX_BYTES every rank (the root) evaluates the vector;
    the in-place Iallreduce evaluates its block and pulls.  (The 32-byte LONG_DOUBLE_INT pair is
    served by gather-then-fold at every size.)"""
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    cases = []
    for count in (7, 65536 // esz - 1):
        xs = [tnbc.make(tname, count, 10 * count + r) for r in range(n)]
        dx = [Buf(torch, xs[r], count, 0, xs[r]) for r in range(n)]
        for inplace in (False, True):
            want, alg = nbc.iallreduce(oracle, op, ty, xs, esz, inplace)
            assert alg == nbc.BINOMIAL
            dr = [Buf(torch, xs[r], count, 0, xs[r]) for r in range(n)] if inplace else [Buf(torch, xs[r], count) for r in range(n)]

            def post(r, dx=dx, dr=dr, count=count, inplace=inplace):
                cs[r].iallreduce(None if inplace else dx[r].ptr, dr[r].ptr, count, ty, op).wait()

            def check(got_alg, dr=dr, want=want, count=count, inplace=inplace):
                assert got_alg == nbc.BINOMIAL
                for r in range(n):
                    what = f"iallreduce n={n} count={count} inplace={inplace} rank={r}"
                    opdata.assert_same(tname, opname, dr[r].get(), want[r], what)
                    assert dr[r].guards_intact(), f"{what}: wrote outside rbuf"

            cases.append((post, check))
        for root in (0, n - 1):
            for inplace in (False, True):
                want, alg = nbc.ireduce(oracle, op, ty, xs, esz, root, inplace)
                assert alg == nbc.BINOMIAL
                dr = Buf(torch, xs[0], count, 0, xs[root] if inplace else None)

                def post(r, dx=dx, dr=dr, count=count, root=root, inplace=inplace):
                    cs[r].ireduce(None if (inplace and r == root) else dx[r].ptr, dr.ptr if r == root else None,
                                  count, ty, op, root).wait()

                def check(got_alg, dr=dr, want=want, count=count, root=root, inplace=inplace):
                    what = f"ireduce n={n} count={count} root={root} inplace={inplace}"
                    assert got_alg == nbc.BINOMIAL
                    opdata.assert_same(tname, opname, dr.get(), want, what)
                    assert dr.guards_intact(), f"{what}: wrote outside rbuf"

                cases.append((post, check))
    with knobs(cs, NB_ORDER=1):
        _run_cases(torch, cs, cases)


# ------------------------------------------------------------------ 3. k_ring_all beyond one chunk
@pytest.mark.parametrize("n", [9, 17, 33])
def test_ring_all(gpu, pkg, oracle, comms, n):
    """ALLREDUCE_ALG 4, not in place, count x size <= ONE_PHASE_MAX_BYTES (1 << 20): every rank
    evaluates every ring block in one k_ring_all launch, n loads in 2, 3 and 5 chunks per element.
    Bit-exact with the oracle's ring and with the two-phase flow (the knob at 0: k_fold +
    k_multicopy); counts n (one element per block), 3n + 1 and 10 007 (ragged partitions)."""
    cs = comms(n)
    with knobs(cs, ALLREDUCE_ALG=4, ONE_PHASE_MAX_BYTES=ONE_PHASE):
        cases, keys = [], []
        for i, slot in enumerate(RING_SLOTS):
            for count in (n, 3 * n + 1, 10_007):
                for one_phase in (ONE_PHASE, 0):
                    cases.append(_allreduce_case(gpu, pkg, oracle, cs, 4, slot, count, False, 7000 + 40 * i,
                                                 one_phase=one_phase))
                    keys.append((slot, count))
        got = _run_cases(gpu, cs, cases)
        for k in range(0, len(got), 2):   # (one launch, two phases) of the same inputs
            (opname, tname), count = keys[k]
            for r in range(n):
                opdata.assert_same(tname, opname, got[k][r], got[k + 1][r], f"ring n={n} count={count} rank={r}: one phase against two")


@pytest.mark.parametrize("slot", tnbc.SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", [9, 17])
def test_ring_all_libnbc(gpu, pkg, oracle, comms, n, slot):
    """NB_ORDER 1, MPI_Iallreduce not in place with count x size just above 65 536: libnbc's ring
    (last_algorithm() 102) in one k_ring_all launch over libnbc's partition -- the NBC instantiation,
    THREE for MAXLOC / MINLOC -- with the last segment short and, at the second count, shorter still"""
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    cases = []
    for count in (65536 // esz + 1, 65536 // esz + n + 3):
        xs = [tnbc.make(tname, count, 11 * count + r) for r in range(n)]
        want, alg = nbc.iallreduce(oracle, op, ty, xs, esz)
        assert alg == nbc.RING
        dx = [Buf(torch, xs[r], count, 0, xs[r]) for r in range(n)]
        dr = [Buf(torch, xs[r], count) for r in range(n)]

        def post(r, dx=dx, dr=dr, count=count):
            cs[r].iallreduce(dx[r].ptr, dr[r].ptr, count, ty, op).wait()

        def check(got_alg, dr=dr, want=want, count=count):
            assert got_alg == nbc.RING
            for r in range(n):
                what = f"libnbc ring n={n} count={count} rank={r}"
                opdata.assert_same(tname, opname, dr[r].get(), want[r], what)
                assert dr[r].guards_intact(), f"{what}: wrote outside rbuf"

        cases.append((post, check))
    with knobs(cs, NB_ORDER=1, ONE_PHASE_MAX_BYTES=ONE_PHASE):
        _run_cases(torch, cs, cases)


# ------------------------------------------------------------------ 4. k_scan_part: the held-back store
SCAN_COUNTS = {"n-1": lambda n: (n - 1, 0), "1000n+7": lambda n: (1000 * n + 7, 0), "50001-shifted": lambda n: (50_001, 1)}


@pytest.mark.parametrize("which", list(SCAN_COUNTS))
@pytest.mark.parametrize("mode", ["blocking", "nb_order1"])
@pytest.mark.parametrize("slot", tscan.SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", [10, 16, 17, 33])
def test_scan_held_back_store(gpu, pkg, oracle, comms, n, slot, mode, which):
    """SCAN_PART_MIN_BYTES 1: every call takes the partitioned flow (last_algorithm() 2), one
    k_scan_part launch per owner over 2, 2, 3 and 5 load chunks.  The case that matters is the
    exclusive scan in place at ranks 8 and 16 (24 and 32 too at n = 33): the prefix after rank 7
    (15, ...) closes a chunk and belongs in rank 8's rbuf, which in place is the input x_8 that the
    next chunk has yet to load, so the store is held back (`pend`) until those loads are issued --
    taken from n = 10 on, with the last prefix closing a chunk (n = 17, 33) and not (10, 16).
    As test_scan_part_gpu: scan and exscan, in place and not, blocking and MPI_Iscan / MPI_Iexscan
    under NB_ORDER 1; counts n - 1, 1000n + 7 (head, 16-byte body and tail in every block) and
    50 001 with the inputs one element past a 16-byte boundary (not in place the outputs stay
    aligned: element-wise).  Against oracle_scan / nbc_scan_oracle and against the chain flow (the
    knob at 0, algorithm 1); rank 0's rbuf keeps every byte after an exscan; guard bytes in front of
    and behind every rbuf.  One reference serves in place and not: the prefixes are the same values,
    and rank 0 of the exclusive form is compared with what it held."""
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    count, shift = SCAN_COUNTS[which](n)
    xs = [tscan.make(tname, count, 100 * count + r) for r in range(n)]
    fill = tscan.make(tname, count, 7)
    cases = []
    for exclusive in (False, True):
        want = tscan._expected(pkg, oracle, mode, exclusive, False, op, ty, xs, fill)
        for inplace in (False, True):
            bufs = []
            for _ in range(2):   # the partitioned flow's buffers and the chain's
                dx = [Buf(torch, xs[r], count, shift * esz, xs[r]) for r in range(n)]
                bufs.append((dx, dx if inplace else [Buf(torch, xs[r], count, 0, fill) for r in range(n)]))
            cases.append((exclusive, inplace, want, bufs))
    algs = {}

    def rank(r):
        torch.cuda.set_device(0)
        c = cs[r]
        for flow, knob in ((0, 1), (1, 0)):
            c.set("SCAN_PART_MIN_BYTES", knob)
            for ci, (exclusive, inplace, _, bufs) in enumerate(cases):
                dx, dr = bufs[flow]
                sp = None if inplace else dx[r].ptr
                if mode == "blocking":
                    (c.exscan if exclusive else c.scan)(sp, dr[r].ptr, count, ty, op)
                else:
                    (c.iexscan if exclusive else c.iscan)(sp, dr[r].ptr, count, ty, op).wait()
                algs[flow, ci, r] = c.last_algorithm()

    torch.cuda.synchronize()
    with knobs(cs, NB_ORDER=1 if mode == "nb_order1" else 0, SCAN_PART_MIN_BYTES=1):
        run_ranks(n, rank)
    torch.cuda.synchronize()
    for ci, (exclusive, inplace, want, bufs) in enumerate(cases):
        what = f"{mode} {'ex' if exclusive else ''}scan n={n} count={count} inplace={inplace}"
        for r in range(n):
            assert algs[0, ci, r] == 2 and algs[1, ci, r] == 1, what
            part, chain = bufs[0][1][r], bufs[1][1][r]
            if exclusive and r == 0:
                before = xs[0] if inplace else fill
                assert part.holds(before) and chain.holds(before), f"{what}: rank 0's rbuf was written"
            else:
                got = part.get()
                opdata.assert_same(tname, opname, got, want[r], f"{what} rank={r}")
                opdata.assert_same(tname, opname, chain.get(), got, f"{what} rank={r}: the chain against the flow")
            assert part.guards_intact() and chain.guards_intact(), f"{what} rank={r}: wrote outside rbuf"


# ------------------------------------------------------------------ 5. every slot once per family
def _fold_slots(pkg, oracle):
    """the slots coll_kernels.hip instantiates (slot_list.hpp): ipc_worker.pipe_all_slots' filter"""
    return [(pkg.OPS[op], pkg.TYPES[ty]) for op in range(1, 13) for ty in range(len(pkg.TYPES))
            if oracle.oracle_has_op(op, ty) and pkg.comm_op_supported(op, ty) and pkg.type_size(ty) <= 16]


def _collect(cases_by_slot, algs):
    bad = []
    for (slot, (_, check)), a in zip(cases_by_slot, algs):
        try:
            check(a)
        except AssertionError as e:
            bad.append(f"{slot[0]}/{slot[1]}: {str(e)[:300]}")
    return bad


@pytest.mark.parametrize("family", ["k_fold", "k_tree", "k_ring_all"])
def test_every_slot_allreduce(gpu, pkg, oracle, comms, family):
    """every (op, type) slot of one kernel family once, at n = 9 and 338 = 37 x 9 + 5 elements, not in
    place: k_fold as ALLREDUCE_ALG 4 with ONE_PHASE_MAX_BYTES 0, k_ring_all the same with the knob
    at 1 << 20, k_tree as ALLREDUCE_ALG 3; mismatches are collected over the slots"""
    n, count = 9, 338
    cs = comms(n)
    alg, one_phase = {"k_fold": (4, 0), "k_ring_all": (4, ONE_PHASE), "k_tree": (3, ONE_PHASE)}[family]
    slots = _fold_slots(pkg, oracle)
    assert len(slots) >= 100, len(slots)
    with knobs(cs, ALLREDUCE_ALG=alg, ONE_PHASE_MAX_BYTES=one_phase):
        cases = [(slot, _allreduce_case(gpu, pkg, oracle, cs, alg, slot, count, False, 5000 + 7 * i))
                 for i, slot in enumerate(slots)]
        algs = run_calls(gpu, cs, [post for _, (post, _) in cases])
    bad = _collect(cases, algs)
    assert not bad, "\n".join(bad[:20])


def test_every_slot_scan(gpu, pkg, oracle, comms):
    """every slot of k_scan_part once: the inclusive scan, not in place, SCAN_PART_MIN_BYTES 1
    (last_algorithm() 2), n = 9, 338 elements, against oracle_scan"""
    torch, n, count = gpu, 9, 338
    cs = comms(n)
    slots = _fold_slots(pkg, oracle)
    assert len(slots) >= 100, len(slots)
    cases = [(slot, _scan_case(torch, pkg, oracle, cs, slot, count, False, False, 6000 + 7 * i)) for i, slot in enumerate(slots)]
    with knobs(cs, SCAN_PART_MIN_BYTES=1):
        algs = run_calls(torch, cs, [post for _, (post, _) in cases])
    bad = _collect(cases, algs)
    assert not bad, "\n".join(bad[:20])


def _scan_case(torch, pkg, oracle, cs, slot, count, exclusive, inplace, salt, sshift=None, rshift=None):
    n = len(cs)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    xs = [opdata.make(tname, count, salt + r) for r in range(n)]
    fill = opdata.make(tname, count, salt + 97)
    want = [x.copy() if inplace else fill.copy() for x in xs]
    assert oracle.oracle_scan(int(exclusive), n, count, ty, op, _ptrs(xs), _ptrs(want)) == 0
    sshift, rshift = sshift or [0] * n, rshift or [0] * n
    dx = [Buf(torch, xs[r], count, sshift[r], xs[r]) for r in range(n)]
    dr = dx if inplace else [Buf(torch, xs[r], count, rshift[r], fill) for r in range(n)]

    def post(r):
        (cs[r].exscan if exclusive else cs[r].scan)(None if inplace else dx[r].ptr, dr[r].ptr, count, ty, op)

    def check(got_alg):
        what = f"{'ex' if exclusive else ''}scan n={n} count={count} inplace={inplace}"
        assert got_alg == 2, what
        for r in range(n):
            if exclusive and r == 0:   # MPI leaves it undefined; the engine leaves it alone
                assert dr[0].holds(xs[0] if inplace else fill), f"{what}: rank 0's rbuf was written"
            else:
                opdata.assert_same(tname, opname, dr[r].get(), want[r], f"{what} rank={r}")
            assert dr[r].guards_intact(), f"{what} rank={r}: wrote outside rbuf"

    return post, check


@pytest.mark.parametrize("opname", ["SUM", "PROD"])
def test_long_double_tree_16(gpu, pkg, oracle, comms, opname):
    """LONG_DOUBLE SUM and PROD (the x87 add and multiply restated in integer arithmetic) through
    k_tree with all 16 registers live: ALLREDUCE_ALG 3 at n = 16, not in place"""
    cs = comms(16)
    with knobs(cs, ALLREDUCE_ALG=3):
        _run_cases(gpu, cs, [_allreduce_case(gpu, pkg, oracle, cs, 3, (opname, "LONG_DOUBLE"), 338, False, 5200)])


# ------------------------------------------------------------------ 5. alignment
def _layout(layout, tname, n):
    """per-rank byte offsets (sbuf, rbuf) past a 16-byte boundary.  align(T) is the C alignment, not
    the size: 4 for FLOAT_INT, 8 for DOUBLE_INT and C_DOUBLE_COMPLEX, so `align` and `mixed` put
    legal MPI buffers at 4 mod 8 and 8 mod 16"""
    dt = opdata.dtype_of(tname)
    a, esz = dt.alignment, dt.itemsize
    if layout == "aligned":
        return [0] * n, [0] * n
    if layout == "head":      # co-misaligned by whole elements where the type allows it: the scalar head peels
        k = esz if esz < 16 else a
        return [k] * n, [k] * n
    if layout == "align":     # the same offset everywhere, one alignment unit: m % sizeof(T) != 0 for the wide types
        return [a] * n, [a] * n
    assert layout == "mixed"  # the operands disagree mod 16: element-wise
    return [(r % 3) * a for r in range(n)], [((r + 1) % 3) * a for r in range(n)]


def test_layouts_reach_the_offsets_named():
    assert [opdata.dtype_of(t).alignment for t in ("FLOAT_INT", "2INT", "SHORT_INT", "C_FLOAT_COMPLEX")] == [4] * 4
    assert [opdata.dtype_of(t).alignment for t in ("DOUBLE_INT", "LONG_INT", "C_DOUBLE_COMPLEX")] == [8] * 3
    assert opdata.dtype_of("LONG_DOUBLE").alignment == 16
    assert _layout("align", "FLOAT_INT", 9)[0][0] % 8 == 4 and _layout("align", "DOUBLE_INT", 9)[0][0] % 16 == 8
    s, r = _layout("mixed", "C_DOUBLE_COMPLEX", 9)
    assert {x % 16 for x in s} == {0, 8} and all(a != b for a, b in zip(s, r))


@pytest.mark.parametrize("layout", ["aligned", "head", "align", "mixed"])
def test_fold_alignment(gpu, pkg, oracle, comms, layout):
    """launch_fold's three branches on the owner-computes allreduce (ALLREDUCE_ALG 4,
    ONE_PHASE_MAX_BYTES 0, not in place, n = 9, 67n + 5 elements): all buffers 16-byte aligned;
    every buffer at the same offset (whole elements: the head peels; one alignment unit of a pair
    or complex type: m % sizeof(T) != 0); rank r's sbuf at (r % 3) x align(T) and its rbuf at
    another multiple (element-wise).  The bytes in front of and behind every rbuf stay untouched."""
    n = 9
    cs = comms(n)
    with knobs(cs, ALLREDUCE_ALG=4, ONE_PHASE_MAX_BYTES=0):
        cases = []
        for i, slot in enumerate(CASES):
            s, r = _layout(layout, slot[1], n)
            cases.append(_allreduce_case(gpu, pkg, oracle, cs, 4, slot, 67 * n + 5, False, 8000 + 40 * i, sshift=s, rshift=r))
        _run_cases(gpu, cs, cases)


@pytest.mark.parametrize("layout", ["aligned", "head", "align", "mixed"])
def test_scan_alignment(gpu, pkg, oracle, comms, layout):
    """launch_scan's branches on the partitioned flow (SCAN_PART_MIN_BYTES 1, n = 9, 67n + 5
    elements), scan and exscan, not in place (sbuf and rbuf at the layout's offsets) and in place;
    guard bytes around every rbuf"""
    torch, n = gpu, 9
    cs = comms(n)
    cases = []
    for i, slot in enumerate(CASES):
        s, r = _layout(layout, slot[1], n)
        for exclusive in (False, True):
            for inplace in (False, True):
                cases.append(_scan_case(torch, pkg, oracle, cs, slot, 67 * n + 5, exclusive, inplace, 9000 + 40 * i,
                                        sshift=s, rshift=r))
    with knobs(cs, SCAN_PART_MIN_BYTES=1):
        _run_cases(torch, cs, cases)


# ------------------------------------------------------------------ 6. past 16 ranks
def test_trees_past_16_ranks_are_refused(gpu, pkg, oracle, comms):
    """n = 17: recursive doubling (ALLREDUCE_ALG 3, and the fixed decision below 10 000 bytes) and
    the binomial reduce (REDUCE_ALG 5) have no device program.  Every rank gets
    MI355X_ERR_UNSUPPORTED, no byte of any rbuf changes, and the ring allreduce that follows on the
    same communicators is exact -- allreduce_impl gives up after its exchange(), which must leave
    no barrier or call number half-done."""
    torch, n, count = gpu, 17, 600
    cs = comms(n)
    tname, opname = "FLOAT", "SUM"
    op, ty = pkg.OP[opname], pkg.T[tname]
    assert oracle.oracle_allreduce_decision(n, count, ty, None) == 3 and count * 4 < 10_000
    xs = [opdata.make(tname, count, 1900 + r) for r in range(n)]
    fill = opdata.make(tname, count, 1899)
    rt = pkg.rt()
    for knob, alg in (("ALLREDUCE_ALG", 3), ("ALLREDUCE_ALG", 0), ("REDUCE_ALG", 5)):
        dx = [Buf(torch, xs[r], count, 0, xs[r]) for r in range(n)]
        dr = [Buf(torch, xs[r], count, 0, fill) for r in range(n)]
        rcs = [None] * n

        def refused(r):
            if knob == "REDUCE_ALG":
                rcs[r] = rt.mi355x_reduce(cs[r].h, dx[r].ptr, dr[r].ptr if r == 0 else None, count, ty, op, 0, None)
            else:
                rcs[r] = rt.mi355x_allreduce(cs[r].h, dx[r].ptr, dr[r].ptr, count, ty, op, None)

        ring = _allreduce_case(torch, pkg, oracle, cs, 4, (opname, tname), count, False, 1950)

        def then_ring(r):
            cs[r].set("ALLREDUCE_ALG", 4)
            ring[0](r)

        with knobs(cs, ALLREDUCE_ALG=alg if knob == "ALLREDUCE_ALG" else 0, REDUCE_ALG=alg if knob == "REDUCE_ALG" else 0):
            algs = run_calls(torch, cs, [refused, then_ring])
        assert rcs == [UNSUPPORTED] * n, (knob, alg, rcs)
        for r in range(n):
            assert dr[r].holds(fill) and dr[r].guards_intact(), f"{knob}={alg}: rank {r}'s rbuf changed"
        ring[1](algs[1])
