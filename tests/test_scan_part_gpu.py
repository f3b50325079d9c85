"""The partitioned MPI_Scan / MPI_Exscan flow on one MI355X: loopback communicators with
SCAN_PART_MIN_BYTES = 1, so every call takes the flow (last_algorithm() == 2): owner q evaluates
ring block q of every rank's prefix in one k_scan_part launch, then every rank pulls its other
blocks out of the owners' scratch.

Blocking, MPI_Iscan and MPI_Iexscan, in place and not, at n = 2, 3, 8 and 9 (9: the exclusive
form's prefix after rank 7 goes to rank 8's block, whose load belongs to the second chunk of
loads).  Counts: 1 (every block but one empty), n - 1, 1000 n + 7 (head, 16-byte body and tail in
every block) and 50 001 with the inputs one element off a 16-byte boundary -- not in place the
outputs stay aligned, so sources and destinations disagree mod 16 and the blocks run element-wise.
Expected bits: coll/basic's chain (oracle_scan) for the blocking calls and for NB_ORDER = 0,
libnbc's schedules (tests/nbc_scan_oracle.py) for NB_ORDER = 1; MAXLOC runs on the tie / NaN pairs
where the two differ.  Every element of every rank is compared bit for bit; rank 0's rbuf after an
exscan holds exactly what it held before.  Every case is then repeated with the knob at 0, which
must report the chain (algorithm 1) and give the same bits.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import nbc_oracle as nbc
import nbc_scan_oracle as nbs
import opdata
from test_nbc_gpu import from_dev, run_ranks, to_dev

pytestmark = pytest.mark.gpu

SLOTS = [("SUM", "FLOAT"), ("SUM", "DOUBLE"), ("MAXLOC", "FLOAT_INT"), ("PROD", "C_DOUBLE_COMPLEX")]
SIZES = [2, 3, 8, 9]
MODES = ["blocking", "nb_order0", "nb_order1"]


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _same_bytes(tname, a, b):
    """every byte of every member equal (a pair type's padding is not the program's; no NaN rule)"""
    return len(opdata.mismatches(tname, "", a, b)) == 0


def make(tname, count, salt):
    dt = opdata.dtype_of(tname)
    if dt.names:
        return nbc.tie_nan_pairs(dt, count, salt)
    if tname in ("FLOAT", "DOUBLE"):
        return np.random.default_rng(0x5CA + 13 * salt).standard_normal(count).astype(dt)
    return opdata.make(tname, count, salt)


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


def _expected(pkg, oracle, mode, exclusive, inplace, op, ty, xs, fill):
    n, count = len(xs), len(xs[0])
    before = [x.copy() if inplace else fill.copy() for x in xs]
    if mode == "nb_order1":
        return nbs.iexscan(oracle, op, ty, xs, before, inplace) if exclusive else nbs.iscan(oracle, op, ty, xs, inplace)
    want = [b.copy() for b in before]
    assert oracle.oracle_scan(int(exclusive), n, count, ty, op, _ptrs(xs), _ptrs(want)) == 0
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slot", SLOTS, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("n", SIZES)
def test_partitioned_scan(gpu, pkg, oracle, comms, n, slot, mode):
    torch, cs = gpu, comms(n)
    opname, tname = slot
    op, ty = pkg.OP[opname], pkg.T[tname]
    esz = pkg.type_size(ty)
    cases = []
    for count, shift in ((1, 0), (n - 1, 0), (1000 * n + 7, 0), (50_001, 1)):
        xs = [make(tname, count, 100 * count + r) for r in range(n)]
        fill = make(tname, count, 7)
        pad = np.zeros(shift, dtype=xs[0].dtype)
        for exclusive in (False, True):
            for inplace in (False, True):
                want = _expected(pkg, oracle, mode, exclusive, inplace, op, ty, xs, fill)
                # two sets of device buffers: the partitioned flow's and the chain's
                bufs = []
                for _ in range(2):
                    dx = [to_dev(torch, np.concatenate([pad, x])) for x in xs]
                    # in place the result buffer is the (shifted) input; else an aligned buffer
                    dr = dx if inplace else [to_dev(torch, fill) for _ in range(n)]
                    bufs.append((dx, dr))
                cases.append((count, shift if inplace else 0, shift, exclusive, inplace, xs, fill, want, bufs))
    algs = {}
    torch.cuda.synchronize()

    def rank(r):
        torch.cuda.set_device(0)
        c = cs[r]
        c.set("NB_ORDER", 1 if mode == "nb_order1" else 0)
        for which, knob in ((0, 1), (1, 0)):
            c.set("SCAN_PART_MIN_BYTES", knob)
            for ci, (count, rshift, sshift, exclusive, inplace, *_rest, bufs) in enumerate(cases):
                dx, dr = bufs[which]
                sp = None if inplace else dx[r].data_ptr() + sshift * esz
                rp = dr[r].data_ptr() + rshift * esz
                if mode == "blocking":
                    (c.exscan if exclusive else c.scan)(sp, rp, count, ty, op)
                else:
                    (c.iexscan if exclusive else c.iscan)(sp, rp, count, ty, op).wait()
                algs[which, ci, r] = c.last_algorithm()

    try:
        run_ranks(n, rank)
    finally:
        for c in cs:
            c.set("NB_ORDER", 0)
            c.set("SCAN_PART_MIN_BYTES", 0)
    torch.cuda.synchronize()
    for ci, (count, rshift, sshift, exclusive, inplace, xs, fill, want, bufs) in enumerate(cases):
        what = f"{mode} {'ex' if exclusive else ''}scan n={n} count={count} inplace={inplace}"
        got = []
        for which in (0, 1):
            dr = bufs[which][1]
            got.append([from_dev(dr[r], xs[0], count + rshift)[rshift:] for r in range(n)])
        for r in range(n):
            assert algs[0, ci, r] == 2 and algs[1, ci, r] == 1, what
            if exclusive and r == 0:
                before = xs[0] if inplace else fill
                assert _same_bytes(tname, got[0][0], before), f"{what}: rank 0's rbuf was written"
            else:
                opdata.assert_same(tname, opname, got[0][r], want[r], f"{what} rank={r}")
            # (the suite's bit comparison, opdata.mismatches: for a float op two NaNs are the same result
            # -- which operand's payload a multiply or an add passes on is the instruction's choice)
            opdata.assert_same(tname, opname, got[1][r], got[0][r], f"{what} rank={r}: the chain against the flow")
            if inplace and sshift:  # the element in front of the shifted buffer is nobody's
                assert not bufs[0][1][r][: sshift * esz].cpu().numpy().any(), f"{what}: wrote in front of rbuf"


@pytest.mark.parametrize("n", [3, 9])
def test_slot_without_a_fold_kernel_keeps_the_chain(gpu, pkg, oracle, comms, n):
    """MAXLOC on the 32-byte LONG_DOUBLE_INT pair is served by gather-then-fold whatever the knob
    says (never algorithm 2), and under NB_ORDER = 1 its Iscan / Iexscan give libnbc's bits"""
    torch, cs = gpu, comms(n)
    opname, tname = "MAXLOC", "LONG_DOUBLE_INT"
    op, ty = pkg.OP[opname], pkg.T[tname]
    count = 301
    xs = [make(tname, count, 40 + r) for r in range(n)]
    fill = make(tname, count, 7)
    want = {False: nbs.iscan(oracle, op, ty, xs), True: nbs.iexscan(oracle, op, ty, xs, [fill] * n)}
    basic = [fill.copy() for _ in range(n)]
    assert oracle.oracle_scan(0, n, count, ty, op, _ptrs(xs), _ptrs(basic)) == 0
    assert len(opdata.mismatches(tname, opname, want[False][n - 1], basic[n - 1])) > 0   # the data tells the rules apart
    dx = [to_dev(torch, x) for x in xs]
    dr = {e: [to_dev(torch, fill) for _ in range(n)] for e in (False, True)}
    algs = {}
    torch.cuda.synchronize()

    def rank(r):
        torch.cuda.set_device(0)
        c = cs[r]
        c.set("NB_ORDER", 1)
        c.set("SCAN_PART_MIN_BYTES", 1)
        c.iscan(dx[r].data_ptr(), dr[False][r].data_ptr(), count, ty, op).wait()
        algs[False, r] = c.last_algorithm()
        c.iexscan(dx[r].data_ptr(), dr[True][r].data_ptr(), count, ty, op).wait()
        algs[True, r] = c.last_algorithm()

    try:
        run_ranks(n, rank)
    finally:
        for c in cs:
            c.set("NB_ORDER", 0)
            c.set("SCAN_PART_MIN_BYTES", 0)
    torch.cuda.synchronize()
    for e in (False, True):
        for r in range(n):
            assert algs[e, r] != 2
            got = from_dev(dr[e][r], xs[0])
            if e and r == 0:
                assert _same_bytes(tname, got, fill), "rank 0's rbuf was written"
            else:
                opdata.assert_same(tname, opname, got, want[e][r], f"exclusive={e} rank={r}")
