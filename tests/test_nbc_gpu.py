"""coll/libnbc's operand order on one MI355X: loopback communicators under NB_ORDER = 1 against the
message-passing simulation of libnbc's schedules (tests/nbc_oracle.py).

MPI_Iallreduce, MPI_Ireduce and MPI_Ireduce_scatter_block, in place and not, at counts on both
sides of libnbc's 64 KiB threshold, for slots whose results expose the order (fp32 SUM), the
operand roles (MAX with NaN and signed zeros) and the 3-buff rule itself (MAXLOC / MINLOC on ties
and NaNs, where no assignment of roles makes the 2-buff rule agree), a complex PROD, and the
32-byte pair the engine serves by gather-then-fold.  Bar: bit-exact (opdata.assert_same), and
last_algorithm() is libnbc's selection.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

import nbc_oracle as nbc
import opdata

pytestmark = pytest.mark.gpu

SLOTS = [("SUM", "FLOAT"), ("MAX", "DOUBLE"), ("MAXLOC", "FLOAT_INT"), ("MINLOC", "DOUBLE_INT"),
         ("PROD", "C_DOUBLE_COMPLEX"), ("MAXLOC", "LONG_DOUBLE_INT")]
SIZES = [2, 3, 4, 5, 8]


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def run_ranks(n, fn):
    errs = [None] * n

    def body(r):
        try:
            fn(r)
        except BaseException as e:  # noqa: BLE001
            errs[r] = e

    th = [threading.Thread(target=body, args=(r,)) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for e in errs:
        if e is not None:
            raise e


def to_dev(torch, a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def from_dev(t, like: np.ndarray, n=None):
    n = len(like) if n is None else n
    return t[: n * like.dtype.itemsize].cpu().numpy().view(like.dtype).copy()


def make(tname, count, salt):
    rng = np.random.default_rng(0xA11 + 31 * salt)
    if tname == "FLOAT":
        return rng.standard_normal(count).astype(np.float32)
    if tname == "DOUBLE":   # MAX: NaNs, zeros of both signs, a few ordinary values
        return rng.choice(np.array([np.nan, -0.0, 0.0, -1.0, 1.0, 2.5]), count)
    dt = opdata.dtype_of(tname)
    if dt.names:
        return nbc.tie_nan_pairs(dt, count, salt)
    return opdata.make(tname, count, salt)


@pytest.fixture(scope="module")
def comms(gpu, pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.Comm.loopback(n, 0)
            for c in made[n]:
                c.set("TIMEOUT_S", 60)
                c.set("NB_ORDER", 1)
        return made[n]

    yield get
    for cs in made.values():
        for c in cs:
            c.destroy()


def _run_calls(torch, cs, n, calls):
    """calls: (post(rank) -> Request, ...) run in order on every rank; returns rank 0's
    last_algorithm() after each"""
    algs = []
    torch.cuda.synchronize()

    def rank(r):
        for post in calls:
            post(r).wait()
            if r == 0:
                algs.append(cs[0].last_algorithm())

    run_ranks(n, rank)
    torch.cuda.synchronize()
    return algs


@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", SIZES)
def test_iallreduce(gpu, pkg, oracle, comms, n, slot):
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    cases, calls = [], []
    for count in (1, 7, 65536 // esz - 1, 65536 // esz + 1):
        for inplace in (False, True):
            xs = [make(tname, count, 10 * count + r) for r in range(n)]
            want, alg = nbc.iallreduce(oracle, op, ty, xs, esz, inplace)
            dx = [to_dev(torch, x) for x in xs]
            dr = [t.clone() if inplace else torch.zeros_like(t) for t in dx]
            cases.append((count, inplace, want, alg, dr))
            calls.append(lambda r, dx=dx, dr=dr, count=count, inplace=inplace: cs[r].iallreduce(
                None if inplace else dx[r].data_ptr(), dr[r].data_ptr(), count, ty, op))
    algs = _run_calls(torch, cs, n, calls)
    for (count, inplace, want, alg, dr), got_alg in zip(cases, algs):
        for r in range(n):
            opdata.assert_same(tname, opname, from_dev(dr[r], want[r]), want[r],
                               f"iallreduce n={n} count={count} inplace={inplace} rank={r}")
        assert got_alg == alg, (count, inplace)
    # both of libnbc's algorithms were seen where it has both
    assert {a for *_, a, _ in cases} == ({nbc.BINOMIAL, nbc.RING} if n >= 4 else {nbc.BINOMIAL})


@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", SIZES)
def test_ireduce(gpu, pkg, oracle, comms, n, slot):
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    cases, calls = [], []
    for count in (1, 7, 65536 // esz - 1, 65536 // esz + 1):
        xs = [make(tname, count, 20 * count + r) for r in range(n)]
        dx = [to_dev(torch, x) for x in xs]
        for root in sorted({0, n // 2, n - 1}):
            for inplace in (False, True):
                want, alg = nbc.ireduce(oracle, op, ty, xs, esz, root, inplace)
                dr = dx[root].clone() if inplace else torch.zeros_like(dx[root])
                cases.append((count, root, inplace, want, alg, dr))
                calls.append(lambda r, dx=dx, dr=dr, count=count, root=root, inplace=inplace: cs[r].ireduce(
                    None if (inplace and r == root) else dx[r].data_ptr(), dr.data_ptr() if r == root else None,
                    count, ty, op, root))
    algs = _run_calls(torch, cs, n, calls)
    for (count, root, inplace, want, alg, dr), got_alg in zip(cases, algs):
        opdata.assert_same(tname, opname, from_dev(dr, want), want,
                           f"ireduce n={n} count={count} root={root} inplace={inplace}")
        assert got_alg == alg, (count, root, inplace)
    assert {c[4] for c in cases} == ({nbc.BINOMIAL, nbc.CHAIN} if n <= 4 else {nbc.BINOMIAL})


@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", SIZES)
def test_ireduce_scatter_block(gpu, pkg, oracle, comms, n, slot):
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    cases, calls = [], []
    for rcount in (1, 301):
        xs = [make(tname, rcount * n, 30 * rcount + r) for r in range(n)]
        want, alg = nbc.ireduce_scatter_block(oracle, op, ty, xs, rcount)
        dx = [to_dev(torch, x) for x in xs]
        dr = [torch.zeros(rcount * xs[0].dtype.itemsize, dtype=torch.uint8, device="cuda") for _ in range(n)]
        cases.append((rcount, want, alg, dr))
        calls.append(lambda r, dx=dx, dr=dr, rcount=rcount: cs[r].ireduce_scatter_block(
            dx[r].data_ptr(), dr[r].data_ptr(), rcount, ty, op))
    algs = _run_calls(torch, cs, n, calls)
    for (rcount, want, alg, dr), got_alg in zip(cases, algs):
        for r in range(n):
            opdata.assert_same(tname, opname, from_dev(dr[r], want[r]), want[r],
                               f"ireduce_scatter_block n={n} rcount={rcount} rank={r}")
        assert got_alg == alg == nbc.BINOMIAL


@pytest.mark.parametrize("n", [3, 4])
def test_order_is_a_knob(gpu, pkg, oracle, comms, n):
    """NB_ORDER = 0 gives coll/tuned's Iallreduce back; a blocking allreduce never depends on it"""
    torch, cs = gpu, comms(n)
    op, ty, count = pkg.OP["SUM"], pkg.T["FLOAT"], 16385
    xs = [make("FLOAT", count, 700 + r) for r in range(n)]
    tuned = [np.zeros_like(xs[0]) for _ in range(n)]
    talg = oracle.oracle_allreduce(0, n, count, ty, op, 0, _ptrs(xs), _ptrs(tuned))
    assert talg >= 0
    libnbc, lalg = nbc.iallreduce(oracle, op, ty, xs, 4)
    assert len(opdata.mismatches("FLOAT", "SUM", libnbc[0], tuned[0])) >= count // 10   # the orders differ
    dx = [to_dev(torch, x) for x in xs]
    out = {k: [torch.zeros_like(t) for t in dx] for k in ("nb1", "blocking", "nb0")}
    algs = {}
    torch.cuda.synchronize()

    def rank(r):
        c = cs[r]
        c.iallreduce(dx[r].data_ptr(), out["nb1"][r].data_ptr(), count, ty, op).wait()
        algs["nb1", r] = c.last_algorithm()
        c.allreduce(dx[r].data_ptr(), out["blocking"][r].data_ptr(), count, ty, op)
        algs["blocking", r] = c.last_algorithm()
        c.set("NB_ORDER", 0)
        assert c.get("NB_ORDER") == 0
        c.iallreduce(dx[r].data_ptr(), out["nb0"][r].data_ptr(), count, ty, op).wait()
        algs["nb0", r] = c.last_algorithm()

    try:
        run_ranks(n, rank)
    finally:
        for c in cs:
            c.set("NB_ORDER", 1)
    torch.cuda.synchronize()
    for r in range(n):
        opdata.assert_same("FLOAT", "SUM", from_dev(out["nb1"][r], xs[0]), libnbc[r], f"NB_ORDER=1 rank={r}")
        opdata.assert_same("FLOAT", "SUM", from_dev(out["blocking"][r], xs[0]), tuned[r], f"blocking rank={r}")
        opdata.assert_same("FLOAT", "SUM", from_dev(out["nb0"][r], xs[0]), tuned[r], f"NB_ORDER=0 rank={r}")
        assert (algs["nb1", r], algs["blocking", r], algs["nb0", r]) == (lalg, talg, talg)


def test_binomial_over_17_ranks_fails_the_post(gpu, pkg, oracle):
    """a libnbc tree the device cannot hold: the posting call returns MI355X_ERR_UNSUPPORTED on every
    rank, nothing is queued, and the communicator still serves what fits"""
    torch = gpu
    n = 17
    cs = pkg.Comm.loopback(n, 0)
    try:
        for c in cs:
            c.set("TIMEOUT_S", 60)
            c.set("NB_ORDER", 1)
        op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
        x = torch.ones(64, dtype=torch.float32, device="cuda")
        y = torch.zeros_like(x)
        torch.cuda.synchronize()
        for fn, args in (("mi355x_iallreduce", (x.data_ptr(), y.data_ptr(), 64, ty, op, None)),
                         ("mi355x_ireduce", (x.data_ptr(), y.data_ptr(), 64, ty, op, 0, None)),
                         ("mi355x_ireduce_scatter_block", (x.data_ptr(), y.data_ptr(), 1, ty, op, None))):
            h = ctypes.c_void_p()
            assert getattr(pkg.rt(), fn)(cs[0].h, *args, ctypes.byref(h)) == -2   # MI355X_ERR_UNSUPPORTED
            assert not h.value
        # the ring fits (a fold): 17 ranks, 64 KiB and more, not in place
        count = 16384 + 5
        xs = [make("FLOAT", count, 900 + r) for r in range(n)]
        want, alg = nbc.iallreduce(oracle, op, ty, xs, 4)
        assert alg == nbc.RING
        dx = [to_dev(torch, a) for a in xs]
        dr = [torch.zeros_like(t) for t in dx]
        torch.cuda.synchronize()
        run_ranks(n, lambda r: cs[r].iallreduce(dx[r].data_ptr(), dr[r].data_ptr(), count, ty, op).wait())
        torch.cuda.synchronize()
        for r in (0, n - 1):
            opdata.assert_same("FLOAT", "SUM", from_dev(dr[r], want[r]), want[r], f"ring at 17 ranks rank={r}")
    finally:
        for c in cs:
            c.destroy()
