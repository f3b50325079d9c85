"""The movement collectives pulling through row layouts of two levels, between processes
(tests/move_planes_worker.py), 3 ranks on one GPU: the engine's mi355x_alltoallv_ddt2 / mi355x_gatherv_ddt2
out of a 3-D subarray and out of interleaved pencils into a two-level receive layout while rank 1 calls the
plain form with dense bytes in the same collective, and the MCA component's MPI_Alltoall of the z-pencils of
a 3-D array of floats with the subarray type on the send side, then on both sides (MOVE_SEND_DIRECT rises on
the engine handle; with coll_mi355x_move_row_levels = 1 the same calls give the same bytes and the counter
stays).  Every result is exact against the numpy model."""
from __future__ import annotations

import os
import pathlib
import subprocess
import sys
import time
import uuid

import pytest

pytestmark = pytest.mark.gpu

HERE = pathlib.Path(__file__).parent
_broken = []   # a worker timed out or died on a signal: nothing more of this module is started on the GPU


def _run(argvs, envs, what):
    """every worker under its own 120 s limit; every rank must exit 0 and print 'rank <r> <what> OK'"""
    if _broken:
        pytest.fail(f"not run: an earlier worker of this module {_broken[0]}")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, str(HERE / "move_planes_worker.py")] + a, env=e,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for a, e in zip(argvs, envs)]
    start = time.monotonic()
    outs, timed_out = [], False
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(0.1, start + 140 - time.monotonic()))
        except subprocess.TimeoutExpired:
            timed_out = True
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    if timed_out or any(p.returncode in (124, 137) for p in procs):
        _broken.append("timed out")
    elif any(p.returncode < 0 or p.returncode in (134, 139) for p in procs):
        _broken.append("died on a signal")
    for r, p in enumerate(procs):
        assert p.returncode == 0 and f"rank {r} {what} OK" in outs[r], f"rank {r} (rc {p.returncode}):\n{outs[r][-3000:]}"


def test_engine_ranks(gpu):
    size, key = 3, "p" + uuid.uuid4().hex[:12]
    env = dict(os.environ, MI355X_TIMEOUT_S="60", MI355X_MOVE_SEND_MIN_RUN="8", MI355X_MOVE_ROW_LEVELS="2")
    _run([["engine", key, str(r), str(size), "0"] for r in range(size)], [env] * size, "engine")


@pytest.mark.parametrize("levels", [2, 1])
def test_component_processes(gpu, levels):
    size, key = 3, uuid.uuid4().hex[:10]
    env = dict(os.environ, MI355X_TIMEOUT_S="60", OMPI_COMM_WORLD_SIZE=str(size), OMPI_COMM_WORLD_LOCAL_SIZE=str(size),
               OMPI_MCA_ess_base_jobid=key, OMPI_MCA_coll_mi355x_move_send_min_run="8",
               OMPI_MCA_coll_mi355x_move_row_levels=str(levels))
    _run([["component", str(r), str(size), key] for r in range(size)],
         [dict(env, OMPI_COMM_WORLD_LOCAL_RANK=str(r), OMPI_COMM_WORLD_RANK=str(r)) for r in range(size)], "component")
