"""CPU tests of MPI_Ireduce_scatter (vector counts) in coll/libnbc's operand order: the schedule
compiler's kind 9, libnbc's decision for coll 3, the test-side simulator (tests/nbc_rs_oracle.py) and
the exported entry points.  Host logic only, no GPU.

The kind-9 program (one per element, the block's owner evaluates it) is interpreted over numpy with
the oracle's 3-buff loop, the way tests/test_nbc_sched.py interprets kind 8, and must equal the
message-passing simulation of nbc_ireduce_scatter.c:84-152 bit for bit -- on ragged counts, where
every block but the first starts at an odd element offset.
"""
from __future__ import annotations

import subprocess

import pytest

import nbc_oracle as nbc
import nbc_rs_oracle as nrs
import opdata
from test_nbc_sched import _data, eval_program3


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8])
def test_equal_counts_are_the_block_schedule(pkg, oracle, n, tname):
    rcount = 5
    opname, op, ty, _, xs = _data(pkg, tname, rcount * n, n, 41)
    for inplace in (False, True):
        want, _ = nbc.ireduce_scatter_block(oracle, op, ty, xs, rcount, inplace)
        got, alg = nrs.ireduce_scatter(oracle, op, ty, xs, [rcount] * n, inplace)
        assert alg == nbc.BINOMIAL
        for r in range(n):
            opdata.assert_same(tname, opname, got[r], want[r], f"n={n} inplace={inplace} rank {r}")


def test_kind_9_is_kind_8(pkg):
    for n in range(2, 17):
        for b in range(n):
            assert pkg.sched_program(9, n, nbc.BINOMIAL, b) == pkg.sched_program(8, n, nbc.BINOMIAL, b), (n, b)


def test_kind_9_over_17_ranks_is_unsupported(pkg):
    with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):
        pkg.sched_program(9, 17, nbc.BINOMIAL, 0)
    with pytest.raises(pkg.MI355XError, match="MI355X_ERR_ARG"):
        pkg.sched_program(9, 4, nbc.BINOMIAL, 4)


@pytest.mark.parametrize("tname", ["FLOAT", "FLOAT_INT"])
@pytest.mark.parametrize("kind", ["ragged", "holes"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 13, 16])
def test_programs_on_ragged_counts(pkg, oracle, n, kind, tname):
    rcounts = nrs.counts_of(kind, n)
    opname, op, ty, _, xs = _data(pkg, tname, sum(rcounts), n, 42)
    outs, _ = nrs.ireduce_scatter(oracle, op, ty, xs, rcounts)
    ins, _ = nrs.ireduce_scatter(oracle, op, ty, xs, rcounts, inplace=True)
    off = 0
    for r in range(n):   # owner-computes: rank r evaluates its program over its own block only
        blk = [x[off:off + rcounts[r]] for x in xs]
        got = eval_program3(oracle, pkg.sched_program(9, n, nbc.BINOMIAL, r), op, ty, blk)
        assert len(outs[r]) == rcounts[r]
        opdata.assert_same(tname, opname, got, outs[r], f"{kind} n={n} rank {r}")
        opdata.assert_same(tname, opname, ins[r], outs[r], f"{kind} in place n={n} rank {r}")
        off += rcounts[r]


def test_decision(pkg):
    for n in range(2, 17):
        for nbytes in (4, 65532, 65536, 1 << 20):
            assert pkg.nbc_decision(3, n, nbytes) == nbc.BINOMIAL
    with pytest.raises(pkg.MI355XError):
        pkg.nbc_decision(4, 4, 64)


@pytest.mark.parametrize("lib,sym", [("libmi355x_rt.so", "mi355x_ireduce_scatter"),
                                     ("mca_coll_mi355x.so", "mca_coll_mi355x_ireduce_scatter")])
def test_exports(pkg, lib, sym):
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(pkg.lib_path(lib))], text=True)
    assert any(line.split()[-1] == sym and line.split()[-2] == "T" for line in out.splitlines() if line.strip()), sym
