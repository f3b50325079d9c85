"""The cross-process flows -- the resident service's LL and pull forms, the per-call LL kernels,
the pipelined allreduce -- on buffers off 16-byte alignment, with guard bytes around every operand
(ipc_worker.py::offalign; the case tables are offalign_plan.py's, and test_offalign_plan.py shows
without a GPU which branches of the device code they enter).

What each size adds: 3 -- an odd tree and a ring with a split; 5 -- the first partial kFoldChunk load
group of the pipelined fold; 8 -- every register of RankRegs and every bit of qmask; 9 -- a second
load group (only the pipelined part has work there: the LL and service forms stop at 8 ranks).
Expected bits: the oracle's schedule simulation; bar: opdata.assert_same.  The worker prints how
many calls every part made; they must equal the counts the plan's tables give, so a part that
silently ran nothing fails.

Part (e) also requires the pipelined result to be byte for byte the two-phase flow's, read as device
bytes (devbuf.Buf.raw: numpy's copy() of a pair type leaves its padding unset).  That check found
what the suite's comparison does not look at: a NaN component of a complex product took its sign
and payload from whichever operand the compiler put first in each kernel (PROD/C_DOUBLE_COMPLEX,
204 bytes in 173 of 1291 elements at 8 ranks, 28 in 24 of 486 at 3); cmul now stores the default
quiet NaN; and the 16-byte vector paths of the two flows stored different bytes in the padding of a
value-index pair (MAXLOC/DOUBLE_INT, 614 bytes in 452 of 486 elements at 3 ranks; the scalar paths
agreed): the padding is now a member that a selected pair carries with it (op_functors.hpp)."""
from __future__ import annotations

import json

import pytest

import offalign_plan as plan
from test_coll_ipc_gpu import _run_mode

pytestmark = pytest.mark.gpu


def expected_calls(size: int, n: dict) -> dict:
    """the plan's own counts, for the limits the worker read from the knobs at run time"""
    want = dict.fromkeys(n, 0)
    want.update(e_pipe=plan.pipe_calls(), e_two_phase=plan.pipe_two_phase_calls())
    if size <= plan.LL_MAX_RANKS:
        served, refused = plan.pull_calls(n["svc_max"])
        want.update(svc_max=n["svc_max"], ll_max=n["ll_max"], pull_max=n["pull_max"],
                    a_red=plan.ll_reduction_calls(size, n["svc_max"]), a_copy=plan.ll_copy_calls(size, n["svc_max"]),
                    b_red=plan.ll_reduction_calls(size, n["ll_max"], algs=(0,), arrangements=("rotated",)),
                    b_copy=plan.ll_copy_calls(size, n["ll_max"]),
                    c_served=served, c_refused=refused, c_back_to_back=plan.PULL_BACK_TO_BACK,
                    d_copy=plan.pull_copy_calls(size, n["svc_max"]), d_rs=plan.rs_calls())
    return want


@pytest.mark.parametrize("size", [3, 5, 8, 9])
def test_offalign(gpu, size):
    outs = _run_mode(gpu, "offalign", size)
    for r, out in enumerate(outs):
        line = next(ln for ln in out.splitlines() if ln.startswith(f"rank {r} offalign calls "))
        n = json.loads(line.split(" calls ", 1)[1])
        assert n == expected_calls(size, n), f"rank {r}: {line}"
        assert n["e_pipe"] > 0 and n["e_two_phase"] > 0
        if size <= plan.LL_MAX_RANKS:
            assert min(n.values()) > 0, line   # every part ran, the refusals of part (c) included
    print(next(ln for ln in outs[0].splitlines() if " offalign calls " in ln))
