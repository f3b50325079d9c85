"""MPI_Ireduce_scatter (vector counts) on one MI355X: loopback communicators under both operand
orders.  NB_ORDER = 1 against the message-passing simulation of libnbc's schedule
(tests/nbc_rs_oracle.py), NB_ORDER = 0 against coll/tuned's three algorithms (the oracle's), the
order as a knob, posting order with the count arrays overwritten after the post, and the 17-rank
hand-off.  Count vectors: the smallest that still exercise the block arithmetic (ragged: every block
but the first starts off a 16-byte boundary; holes, one owner and empty: ranks that receive nothing
still contribute).  Bar: bit-exact (opdata.assert_same), bytes of rbuf beyond the rank's block
untouched, last_algorithm() the order's.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import nbc_oracle as nbc
import nbc_rs_oracle as nrs
import opdata
from test_nbc_gpu import SIZES, SLOTS, _ptrs, from_dev, make, run_ranks, to_dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 64   # sentinel bytes past the whole vector (an empty vector still has bytes to check)


@pytest.fixture(scope="module")
def comms(gpu, pkg):
    made = {}

    def get(n, order):
        if n not in made:
            made[n] = pkg.Comm.loopback(n, 0)
            for c in made[n]:
                c.set("TIMEOUT_S", 60)
        for c in made[n]:
            c.set("NB_ORDER", order)
            c.set("REDUCE_SCATTER_ALG", 0)
        return made[n]

    yield get
    for cs in made.values():
        for c in cs:
            c.destroy()


def _tuned(oracle, alg, ty, op, xs, rcounts):
    """coll/tuned's reduce_scatter (alg 0: its fixed decision): (every rank's block, the algorithm)"""
    n = len(xs)
    vp, i = ctypes.c_void_p, ctypes.c_int
    oracle.oracle_reduce_scatter.argtypes = [i, ctypes.POINTER(i), i, i, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    outs = [np.zeros(max(c, 1), dtype=xs[0].dtype) for c in rcounts]
    rc = (ctypes.c_int * n)(*rcounts)
    if alg:
        got = oracle.oracle_reduce_scatter_alg(alg, n, rc, ty, op, _ptrs(xs), _ptrs(outs))
    else:
        got = oracle.oracle_reduce_scatter(n, rc, ty, op, _ptrs(xs), _ptrs(outs))
    assert got >= 0
    return [o[:c] for o, c in zip(outs, rcounts)], got


class _Case:
    """one call on every rank: device buffers, the post, the checks"""

    def __init__(self, torch, xs, rcounts, inplace, want, what):
        self.rcounts, self.inplace, self.want, self.what = rcounts, inplace, want, what
        self.esz = xs[0].dtype.itemsize
        total = sum(rcounts)
        # (an empty vector: a send buffer all the same, so that sbuf is not MPI_IN_PLACE)
        self.dx = [to_dev(torch, x) if total else torch.zeros(16, dtype=torch.uint8, device="cuda") for x in xs]
        if inplace:   # the whole vector is in rbuf; the guard follows it
            self.dr = [torch.cat([to_dev(torch, x), torch.full((GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")])
                       for x in xs]
        else:
            self.dr = [torch.full((total * self.esz + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in xs]

    def post(self, cs, r, ty, op, counts=None):
        sp = None if self.inplace else self.dx[r].data_ptr()
        return cs[r].ireduce_scatter(sp, self.dr[r].data_ptr(), self.rcounts if counts is None else counts, ty, op)

    def check(self, tname, opname):
        total = sum(self.rcounts)
        for r, k in enumerate(self.rcounts):
            raw = self.dr[r].cpu().numpy()
            got = raw[: k * self.esz].view(self.want[r].dtype)
            opdata.assert_same(tname, opname, got, self.want[r], f"{self.what} rank={r}")
            if self.inplace:   # the rest of the input vector is the engine's to leave; the guard is not
                assert (raw[total * self.esz:] == SENTINEL).all(), f"{self.what} rank={r}: wrote past the vector"
            else:
                assert (raw[k * self.esz:] == SENTINEL).all(), f"{self.what} rank={r}: wrote past its block"


def _run(torch, cs, cases, ty, op):
    """every case posted and waited in order on every rank; rank 0's last_algorithm() after each"""
    algs = []
    torch.cuda.synchronize()

    def rank(r):
        for case in cases:
            case.post(cs, r, ty, op).wait()
            if r == 0:
                algs.append(cs[0].last_algorithm())

    run_ranks(len(cs), rank)
    torch.cuda.synchronize()
    return algs


@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", SIZES)
def test_libnbc_order(gpu, pkg, oracle, comms, n, slot):
    torch, cs = gpu, comms(n, 1)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    cases = []
    for vi, kind in enumerate(nrs.VECTORS):
        rcounts = nrs.counts_of(kind, n)
        xs = [make(tname, sum(rcounts), 40 * vi + r) for r in range(n)]
        for inplace in (False, True):
            if sum(rcounts):
                want, alg = nrs.ireduce_scatter(oracle, op, ty, xs, rcounts, inplace)
                assert alg == nbc.BINOMIAL
            else:
                want = [x[:0] for x in xs]
            cases.append(_Case(torch, xs, rcounts, inplace, want, f"NB_ORDER=1 n={n} {kind} inplace={inplace}"))
    algs = _run(torch, cs, cases, ty, op)
    for case, alg in zip(cases, algs):
        case.check(tname, opname)
        if sum(case.rcounts):
            assert alg == nbc.BINOMIAL, case.what


@pytest.mark.parametrize("slot", [("SUM", "FLOAT"), ("MAXLOC", "FLOAT_INT")], ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("rsalg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_tuned_order(gpu, pkg, oracle, comms, n, rsalg, slot):
    torch, cs = gpu, comms(n, 0)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    cases, walgs = [], []
    for vi, kind in enumerate(("ragged", "holes")):
        rcounts = nrs.counts_of(kind, n)
        xs = [make(tname, sum(rcounts), 50 * vi + r) for r in range(n)]
        want, walg = _tuned(oracle, rsalg, ty, op, xs, rcounts)
        for inplace in (False, True):
            cases.append(_Case(torch, xs, rcounts, inplace, want, f"NB_ORDER=0 alg={rsalg} n={n} {kind} inplace={inplace}"))
            walgs.append(walg)
    for c in cs:
        c.set("REDUCE_SCATTER_ALG", rsalg)
    try:
        algs = _run(torch, cs, cases, ty, op)
    finally:
        for c in cs:
            c.set("REDUCE_SCATTER_ALG", 0)
    for case, alg, walg in zip(cases, algs, walgs):
        case.check(tname, opname)
        if sum(case.rcounts):   # (holes over 2 ranks is the empty vector: nothing ran)
            assert alg == walg and (rsalg == 0 or alg == rsalg), case.what


@pytest.mark.parametrize("n", [3, 4, 5])
def test_order_is_a_knob(gpu, pkg, oracle, comms, n):
    torch = gpu
    opname, tname = "SUM", "FLOAT"
    op, ty = pkg.OP[opname], pkg.T[tname]
    rcounts = [1367] * n
    xs = [make(tname, sum(rcounts), 800 + r) for r in range(n)]
    libnbc, _ = nrs.ireduce_scatter(oracle, op, ty, xs, rcounts)
    tuned, talg = _tuned(oracle, 0, ty, op, xs, rcounts)
    # a condition of the test, checked on the CPU: the two orders give different bits on these inputs
    differ = sum(len(opdata.mismatches(tname, opname, libnbc[r], tuned[r])) for r in range(n))
    assert differ >= sum(rcounts) // 20, f"seed 800: only {differ} elements tell the orders apart"
    for order, want, walg in ((1, libnbc, nbc.BINOMIAL), (0, tuned, talg), (1, libnbc, nbc.BINOMIAL)):
        cs = comms(n, order)
        case = _Case(torch, xs, rcounts, False, want, f"knob NB_ORDER={order} n={n}")
        assert _run(torch, cs, [case], ty, op) == [walg]
        case.check(tname, opname)


@pytest.mark.parametrize("order", [0, 1])
def test_posting_order_and_copied_counts(gpu, pkg, oracle, comms, order):
    """ireduce_scatter(A), iallreduce, ireduce_scatter(B) posted back to back, the count arrays
    overwritten right after the posts, waited in reverse order"""
    torch, n = gpu, 4
    cs = comms(n, order)
    opname, tname = "SUM", "FLOAT"
    op, ty = pkg.OP[opname], pkg.T[tname]
    ca, cb = nrs.counts_of("ragged", n), nrs.counts_of("holes", n)
    cb[1] += 2   # (B's total differs from A's)
    xa = [make(tname, sum(ca), 900 + r) for r in range(n)]
    xb = [make(tname, sum(cb), 910 + r) for r in range(n)]
    count = 4099
    xr = [make(tname, count, 920 + r) for r in range(n)]
    if order:
        wa, _ = nrs.ireduce_scatter(oracle, op, ty, xa, ca)
        wb, _ = nrs.ireduce_scatter(oracle, op, ty, xb, cb)
        wr, _ = nbc.iallreduce(oracle, op, ty, xr, 4)
    else:
        wa, _ = _tuned(oracle, 0, ty, op, xa, ca)
        wb, _ = _tuned(oracle, 0, ty, op, xb, cb)
        wr = [np.zeros_like(xr[0]) for _ in range(n)]
        assert oracle.oracle_allreduce(0, n, count, ty, op, 0, _ptrs(xr), _ptrs(wr)) >= 0
    A = _Case(torch, xa, ca, False, wa, f"A NB_ORDER={order}")
    B = _Case(torch, xb, cb, False, wb, f"B NB_ORDER={order}")
    dxr = [to_dev(torch, x) for x in xr]
    drr = [torch.zeros_like(t) for t in dxr]
    torch.cuda.synchronize()

    def rank(r):
        arr_a, arr_b = (ctypes.c_int * n)(*ca), (ctypes.c_int * n)(*cb)
        qa = A.post(cs, r, ty, op, arr_a)
        qr = cs[r].iallreduce(dxr[r].data_ptr(), drr[r].data_ptr(), count, ty, op)
        qb = B.post(cs, r, ty, op, arr_b)
        for j in range(n):   # the engine copied the counts at the post
            arr_a[j] = -12345 - j
            arr_b[j] = 0x7FFFFFF0 + j
        for q in (qb, qr, qa):
            q.wait()

    run_ranks(n, rank)
    torch.cuda.synchronize()
    A.check(tname, opname)
    B.check(tname, opname)
    for r in range(n):
        opdata.assert_same(tname, opname, from_dev(drr[r], wr[r]), wr[r], f"iallreduce between them rank={r}")


def test_binomial_over_17_ranks_fails_the_post(gpu, pkg):
    """libnbc's tree over 17 ranks does not fit the device: the posting call returns
    MI355X_ERR_UNSUPPORTED on every rank and nothing is queued"""
    torch = gpu
    n = 17
    cs = pkg.Comm.loopback(n, 0)
    try:
        for c in cs:
            c.set("TIMEOUT_S", 60)
            c.set("NB_ORDER", 1)
        op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
        x = torch.ones(n, dtype=torch.float32, device="cuda")
        y = torch.zeros_like(x)
        torch.cuda.synchronize()
        counts = (ctypes.c_int * n)(*([1] * n))
        for c in cs:
            h = ctypes.c_void_p()
            rc = pkg.rt().mi355x_ireduce_scatter(c.h, x.data_ptr(), y.data_ptr(), counts, ty, op, None, ctypes.byref(h))
            assert rc == -2 and not h.value   # MI355X_ERR_UNSUPPORTED
        for c in cs:   # nothing is pending: the knob may change (it may not while a call is queued)
            c.set("NB_ORDER", 0)
        torch.cuda.synchronize()
        assert (y.cpu().numpy() == 0).all()
    finally:
        for c in cs:
            c.destroy()
