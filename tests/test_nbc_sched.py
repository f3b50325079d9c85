"""CPU tests of coll/libnbc's operand order in the schedule compiler (host logic, no GPU).

The per-element programs the engine runs for MPI_Iallreduce / MPI_Ireduce /
MPI_Ireduce_scatter_block under NB_ORDER = 1 (mi355x_sched_program kinds 6-8) are interpreted here
over numpy with the oracle's 3-buff loop and must equal, bit for bit, the message-passing
simulation of libnbc's schedules (tests/nbc_oracle.py).  fp32 SUM on N(0,1) data shows every
difference of order; MAXLOC on ties and NaNs shows every difference of operand role and of the
2-buff against the 3-buff rule.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import nbc_oracle as nbc
import opdata

SIZES = [2, 3, 4, 5, 6, 7, 8, 13, 16]
ERR_UNSUPPORTED = -2


def eval_program3(oracle, prog, op, ty, xs):
    """a serialized libnbc program: every step is op3(in1 = the `out` slot, in2 = the `in` slot)"""
    def op3(a, b):
        out = a.copy()
        a, b = np.ascontiguousarray(a).copy(), np.ascontiguousarray(b).copy()
        oracle.oracle_op_3buff(op, ty, a.ctypes.data, b.ctypes.data, out.ctypes.data, len(out))
        return out
    assert prog[0] in (2, 3), "kinds 6-8 report the 3-buff rule (layout id + 2)"
    if prog[0] == 3:
        L = prog[2]
        order, roles = prog[3:3 + L], prog[3 + L:3 + 2 * L]
        acc = xs[order[0]].copy()
        for j in range(1, L):
            acc = op3(acc, xs[order[j]]) if roles[j] else op3(xs[order[j]], acc)
        return acc
    nsteps, result = prog[2], prog[3]
    R = [x.copy() for x in xs]
    for k in range(nsteps):
        d, o, i = prog[4 + 3 * k: 7 + 3 * k]
        R[d] = op3(R[o], R[i])
    return R[result]


def _data(pkg, tname, count, n, salt):
    """(op name, op, type, element size, n inputs)"""
    if tname == "FLOAT":
        rng = np.random.default_rng(1000 * salt + n)
        return "SUM", pkg.OP["SUM"], pkg.T[tname], 4, [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    dt = opdata.dtype_of(tname)
    return "MAXLOC", pkg.OP["MAXLOC"], pkg.T[tname], dt.itemsize, [nbc.tie_nan_pairs(dt, count, 100 * salt + r)
                                                                for r in range(n)]


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("n", SIZES)
def test_iallreduce_programs(pkg, oracle, n, tname):
    count = 61
    opname, op, ty, esz, xs = _data(pkg, tname, count, n, 1)
    outs, alg = nbc.iallreduce(oracle, op, ty, xs, esz)
    assert alg == nbc.BINOMIAL
    for r in range(1, n):
        opdata.assert_same(tname, opname, outs[r], outs[0], f"ranks agree n={n}")
    got = eval_program3(oracle, pkg.sched_program(6, n, nbc.BINOMIAL, 0), op, ty, xs)
    opdata.assert_same(tname, opname, got, outs[0], f"binomial n={n}")
    ins, _ = nbc.iallreduce(oracle, op, ty, xs, esz, inplace=True)
    opdata.assert_same(tname, opname, ins[n - 1], outs[0], f"in place gives the same expression n={n}")
    # the ring: every segment, over libnbc's partition (uneven: the last segment is short)
    count = 16 * n + 3
    opname, op, ty, esz, xs = _data(pkg, tname, count, n, 2)
    outs, alg = nbc.iallreduce(oracle, op, ty, xs, esz, alg=nbc.RING)
    for r in range(1, n):
        opdata.assert_same(tname, opname, outs[r], outs[0], f"ring ranks agree n={n}")
    for e, (lo, ln) in enumerate(nbc.ring_segments(count, n)):
        assert pkg.nbc_ring_block(count, n, e) == (lo, ln)
        got = eval_program3(oracle, pkg.sched_program(6, n, nbc.RING, e), op, ty, [x[lo:lo + ln] for x in xs])
        opdata.assert_same(tname, opname, got, outs[0][lo:lo + ln], f"ring n={n} segment {e}")


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("n", SIZES)
def test_ireduce_programs(pkg, oracle, n, tname):
    count = 67
    opname, op, ty, esz, xs = _data(pkg, tname, count, n, 3)
    for root in range(n):
        for alg in (nbc.BINOMIAL, nbc.CHAIN):
            want, _ = nbc.ireduce(oracle, op, ty, xs, esz, root, alg=alg)
            got = eval_program3(oracle, pkg.sched_program(7, n, alg, root), op, ty, xs)
            opdata.assert_same(tname, opname, got, want, f"ireduce alg={alg} n={n} root={root}")
        inp, _ = nbc.ireduce(oracle, op, ty, xs, esz, root, inplace=True, alg=nbc.BINOMIAL)
        want, _ = nbc.ireduce(oracle, op, ty, xs, esz, root, alg=nbc.BINOMIAL)
        opdata.assert_same(tname, opname, inp, want, f"in place at the root n={n} root={root}")


def test_ireduce_chain_fragments(pkg, oracle):
    """the chain as libnbc selects it (>= 64 KiB, <= 4 ranks): its 8 KiB fragments change no element's order"""
    n, count = 4, 16385
    opname, op, ty, esz, xs = _data(pkg, "FLOAT", count, n, 4)
    for root in range(n):
        want, alg = nbc.ireduce(oracle, op, ty, xs, esz, root)
        assert alg == nbc.CHAIN
        got = eval_program3(oracle, pkg.sched_program(7, n, nbc.CHAIN, root), op, ty, xs)
        opdata.assert_same("FLOAT", opname, got, want, f"chain root={root}")


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("n", SIZES)
def test_ireduce_scatter_block_programs(pkg, oracle, n, tname):
    rcount = 5
    opname, op, ty, esz, xs = _data(pkg, tname, rcount * n, n, 5)
    outs, _ = nbc.ireduce_scatter_block(oracle, op, ty, xs, rcount)
    ins, _ = nbc.ireduce_scatter_block(oracle, op, ty, xs, rcount, inplace=True)
    got = eval_program3(oracle, pkg.sched_program(8, n, 0, 0), op, ty, xs)
    for r in range(n):
        opdata.assert_same(tname, opname, got[r * rcount:(r + 1) * rcount], outs[r], f"rsb n={n} rank {r}")
        opdata.assert_same(tname, opname, ins[r], outs[r], f"rsb in place n={n} rank {r}")


def test_decisions(pkg):
    B, R, C = nbc.BINOMIAL, nbc.RING, nbc.CHAIN
    d = pkg.nbc_decision
    # MPI_Iallreduce: binomial when p < 4 || bytes < 65536 || in place, else ring
    assert [d(0, p, 65536) for p in (3, 4, 5)] == [B, R, R]
    assert [d(0, p, 65532) for p in (3, 4, 5)] == [B, B, B]
    assert [d(0, p, 65536, True) for p in (3, 4, 5)] == [B, B, B]
    assert d(0, 64, 1 << 30) == R
    # MPI_Ireduce: binomial when p > 4 || bytes < 65536, else chain
    assert [d(1, p, 65536) for p in (3, 4, 5)] == [C, C, B]
    assert [d(1, p, 65532) for p in (3, 4, 5)] == [B, B, B]
    # MPI_Ireduce_scatter_block: always the binomial
    assert [d(2, p, 1 << 20) for p in (3, 4, 5)] == [B, B, B]
    # ... and they are the simulator's
    for p in (2, 3, 4, 5, 8):
        for nbytes in (4, 65532, 65536, 1 << 20):
            for inplace in (False, True):
                assert d(0, p, nbytes, inplace) == nbc.iallreduce_alg(p, nbytes // 4, 4, inplace)
            assert d(1, p, nbytes) == nbc.ireduce_alg(p, nbytes // 4, 4)


def test_binomial_over_17_ranks_is_unsupported(pkg):
    """a tree program holds 16 ranks: the binomial at 17 does not compile (the post call then returns
    MI355X_ERR_UNSUPPORTED instead of queueing a call that cannot run)"""
    buf = (ctypes.c_int * 4096)()
    for kind, alg in ((6, nbc.BINOMIAL), (7, nbc.BINOMIAL), (8, 0)):
        assert pkg.rt().mi355x_sched_program(kind, 16, alg, 0, buf, 4096) > 0
        assert pkg.rt().mi355x_sched_program(kind, 17, alg, 0, buf, 4096) == ERR_UNSUPPORTED
    # the folds fit any communicator the engine takes
    assert pkg.rt().mi355x_sched_program(6, 64, nbc.RING, 63, buf, 4096) > 0
    assert pkg.rt().mi355x_sched_program(7, 64, nbc.CHAIN, 5, buf, 4096) > 0


@pytest.mark.parametrize("count,p", [(16385, 4), (16385, 5), (2049, 64), (10, 4)])
def test_ring_partition(pkg, count, p):
    segsize = -(-count // p)
    blocks = [pkg.nbc_ring_block(count, p, e) for e in range(p)]
    assert blocks == nbc.ring_segments(count, p)
    assert sum(ln for _, ln in blocks) == count
    pos = 0
    for off, ln in blocks:                       # contiguous and in order
        assert off == pos and 0 <= ln <= segsize
        pos += ln
    full = count // segsize
    assert [ln for _, ln in blocks[:full]] == [segsize] * full
    if full < p:                                 # a short one, then empty ones
        assert blocks[full][1] == count - full * segsize
        assert all(ln == 0 for _, ln in blocks[full + 1:])
    if (count, p) == (2049, 64):
        assert blocks[62][1] == 3 and blocks[63][1] == 0
    if (count, p) == (10, 4):
        assert [ln for _, ln in blocks] == [3, 3, 3, 1]


@pytest.mark.parametrize("n", [3, 4, 5])
def test_libnbc_order_differs_from_tuned(pkg, oracle, n):
    """what makes the GPU tests meaningful: on fp32 SUM the two components' results differ in a
    large share of the elements, so coll/tuned's order cannot pass for libnbc's"""
    count = 16385
    _, op, ty, esz, xs = _data(pkg, "FLOAT", count, n, 6)
    want, _ = nbc.iallreduce(oracle, op, ty, xs, esz)
    outs = [np.zeros_like(xs[0]) for _ in range(n)]
    ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    assert oracle.oracle_allreduce(0, n, count, ty, op, 0, ptrs(xs), ptrs(outs)) >= 0
    differ = int((want[0].view(np.uint32) != outs[0].view(np.uint32)).sum())
    print(f"n={n}: {differ} of {count} elements differ ({100.0 * differ / count:.1f} %)")
    assert differ >= count // 10
