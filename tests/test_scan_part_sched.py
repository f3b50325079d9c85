"""CPU tests of the partitioned MPI_Scan / MPI_Exscan flow's host side and of the nonblocking scan
slots (no GPU needed):

* mi355x_scan_part_plan -- the layout the flow and these tests share: the owners' blocks tile the
  vector, one owner's slots do not overlap and fit the scratch the flow asks for;
* the SCAN_PART_MIN_BYTES knob;
* tests/nbc_scan_oracle.py, the restatement of libnbc's Iscan / Iexscan schedules, against the
  chain written out with the oracle's 3-buff loop, and against coll/basic's chain (oracle_scan) on
  the MAXLOC pairs where the 2-buff and 3-buff rules differ;
* coll/mi355x installs MPI_Iscan and MPI_Iexscan.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import nbc_oracle as nbc
import nbc_scan_oracle as nbs
import opdata
from mini import mini

SIZES = list(range(1, 10)) + [10, 16, 17, 33]   # 10: the first size whose exclusive form holds a store back


def _counts(n):
    return sorted({0, 1, n - 1, n, 1000 * n + 7})


@pytest.mark.parametrize("n", SIZES)
def test_plan_tiles_and_slots_fit(pkg, n):
    for count in _counts(n):
        pos = 0
        for q in range(n):
            off, ln, slot = pkg.scan_part_plan(count, n, q, q)
            assert slot is None                      # the owner's own prefix goes straight to its rbuf
            assert off == pos, (count, q)            # the blocks tile [0, count) in rank order
            pos += ln
            taken = []
            for r in range(n):
                o2, l2, s2 = pkg.scan_part_plan(count, n, q, r)
                assert (o2, l2) == (off, ln)
                if r != q:
                    taken.append((s2, s2 + ln))
            taken.sort()
            for (a0, a1), (b0, b1) in zip(taken, taken[1:]):
                assert a1 <= b0, (count, q)          # one owner's slots do not overlap
            need = max((e for _, e in taken), default=0) if ln else 0
            # what the flow asks ensure_scratch for: n - 1 slots of the block's length
            assert need == (n - 1) * ln
            # The slots fit in count elements of scratch -- except at count = 1 with n >= 3, where
            # no layout can: owner 0 holds the one element of n - 1 other ranks' prefixes.  There
            # the bound is what those prefixes need, n - 1 elements.
            if count == 1 and n >= 3:
                assert need == (n - 1 if q == 0 else 0)
            else:
                assert need <= count, (count, n, q)
        assert pos == count


def test_plan_rejects_bad_arguments(pkg):
    for args in ((10, 0, 0, 0), (10, 65, 0, 0), (10, 4, 4, 0), (10, 4, 0, -1)):
        with pytest.raises(pkg.MI355XError, match="bad scan plan arguments"):
            pkg.scan_part_plan(*args)


def test_knob_round_trips(pkg):
    assert pkg.KNOB["SCAN_PART_MIN_BYTES"] == 45
    cs = pkg.Comm.loopback(2, 0)
    try:
        for v in (0, 1, 65536, 1 << 40):
            for c in cs:
                c.set("SCAN_PART_MIN_BYTES", v)
                assert c.get("SCAN_PART_MIN_BYTES") == v
        with pytest.raises(pkg.MI355XError, match="scan_part_min_bytes out of range"):
            cs[0].set("SCAN_PART_MIN_BYTES", -1)
        assert cs[0].get("SCAN_PART_MIN_BYTES") == 1 << 40     # a rejected value changes nothing
    finally:
        for c in cs:
            c.destroy()


def _data(pkg, tname, count, n, salt):
    if tname == "FLOAT":
        rng = np.random.default_rng(77 * salt + n)
        return "SUM", [rng.standard_normal(count).astype(np.float32) for _ in range(n)]
    dt = opdata.dtype_of(tname)
    return "MAXLOC", [nbc.tie_nan_pairs(dt, count, 50 * salt + r) for r in range(n)]


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
def test_libnbc_scan_oracle_is_the_3buff_chain(pkg, oracle, n, tname):
    count = 203
    opname, xs = _data(pkg, tname, count, n, 1)
    op, ty = pkg.OP[opname], pkg.T[tname]
    fill = np.frombuffer(bytes([0xA5]) * xs[0].nbytes, dtype=xs[0].dtype)
    for inplace in (False, True):
        inc = nbs.iscan(oracle, op, ty, xs, inplace)
        exc = nbs.iexscan(oracle, op, ty, xs, [fill] * n, inplace)
        for r in range(n):
            want = nbs.chain3(oracle, op, ty, xs, r)
            opdata.assert_same(tname, opname, inc[r], want, f"iscan n={n} rank={r} inplace={inplace}")
            if r + 1 < n:   # rank r + 1 of the exclusive form holds rank r's inclusive result
                opdata.assert_same(tname, opname, exc[r + 1], want, f"iexscan n={n} rank={r + 1} inplace={inplace}")
        # rank 0's recvbuf is never written
        assert exc[0].tobytes() == (xs[0] if inplace else fill).tobytes()


@pytest.mark.parametrize("n", [2, 3, 8, 9])
def test_libnbc_scan_differs_from_coll_basic_on_ties_and_nans(pkg, oracle, n):
    count = 4000
    opname, xs = _data(pkg, "FLOAT_INT", count, n, 2)
    op, ty = pkg.OP[opname], pkg.T["FLOAT_INT"]
    basic = [np.zeros_like(xs[0]) for _ in range(n)]
    ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])  # noqa: E731
    assert oracle.oracle_scan(0, n, count, ty, op, ptrs(xs), ptrs(basic)) == 0
    libnbc = nbs.iscan(oracle, op, ty, xs)
    assert len(opdata.mismatches("FLOAT_INT", opname, libnbc[0], basic[0])) == 0   # rank 0: a copy either way
    for r in range(1, n):
        assert len(opdata.mismatches("FLOAT_INT", opname, libnbc[r], basic[r])) > 0, f"rank {r}: the two rules agree"
    # and on fp32 SUM the two chains are the same expression
    opname, xs = _data(pkg, "FLOAT", count, n, 3)
    op, ty = pkg.OP[opname], pkg.T["FLOAT"]
    basic = [np.zeros_like(xs[0]) for _ in range(n)]
    assert oracle.oracle_scan(0, n, count, ty, op, ptrs(xs), ptrs(basic)) == 0
    libnbc = nbs.iscan(oracle, op, ty, xs)
    for r in range(n):
        opdata.assert_same("FLOAT", opname, libnbc[r], basic[r], f"SUM rank {r}")


def test_component_installs_iscan_and_iexscan(monkeypatch):
    m = mini()
    monkeypatch.setenv("OMPI_COMM_WORLD_SIZE", "4")
    monkeypatch.setenv("OMPI_COMM_WORLD_LOCAL_SIZE", "4")

    class CollComp(ctypes.Structure):
        _fields_ = [("version", ctypes.c_char * 200), ("data", ctypes.c_char * 36),
                    ("init_query", ctypes.c_void_p), ("comm_query", ctypes.c_void_p)]

    comp = CollComp.from_address(m.component_ptr(m.coll, "mca_coll_mi355x_component"))
    query = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int))(comp.comm_query)
    comm = m.lib.mini_comm_create(0, 4, 77)
    assert m.lib.mini_comm_fn(comm, 20) is None and m.lib.mini_comm_fn(comm, 21) is None
    prio = ctypes.c_int(-1)
    mod = query(comm, ctypes.byref(prio))
    assert mod and prio.value == 90
    m.lib.mini_comm_install(comm, mod)
    assert m.lib.mini_comm_fn(comm, 20) == m.addr(m.coll, "mca_coll_mi355x_iscan")
    assert m.lib.mini_comm_fn(comm, 21) == m.addr(m.coll, "mca_coll_mi355x_iexscan")
    # the blocking slots next to them are the ones they were
    assert m.lib.mini_comm_fn(comm, 18) == m.addr(m.coll, "mca_coll_mi355x_scan")
    assert m.lib.mini_comm_fn(comm, 19) == m.addr(m.coll, "mca_coll_mi355x_exscan")
    m.lib.mini_comm_destroy(comm)
    # the host module gives the slots a fallback of its own
    host = m.lib.mini_comm_create(0, 4, 78)
    m.lib.mini_host_module.restype = ctypes.c_void_p
    hm = m.lib.mini_host_module()
    m.lib.mini_comm_install(host, hm)
    assert m.lib.mini_comm_fn(host, 20) and m.lib.mini_comm_fn(host, 21)
    assert m.lib.mini_comm_fn(host, 20) != m.lib.mini_comm_fn(host, 21)
    m.lib.mini_comm_destroy(host)
