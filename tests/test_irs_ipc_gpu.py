"""MPI_Ireduce_scatter (vector counts) between processes (tests/irs_worker.py), 3 ranks on one GPU:
the engine's C ABI under both NB_ORDER values -- ragged counts, ranks that receive nothing, a
60 001-element-per-rank vector, in place and not, libnbc's order on MAXLOC ties and NaNs -- and the
MCA component under coll_mi355x_nb_order 0 and 1: the slot is the component's, device buffers and
host buffers on every rank (which join the engine) are exact for that order, and a user-defined op
is staged to the lower-priority module, which never sees a device pointer.  Every result is
compared bit for bit."""
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
    procs = [subprocess.Popen([sys.executable, str(HERE / "irs_worker.py")] + a, env=e, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for a, e in zip(argvs, envs)]
    start = time.monotonic()
    outs, timed_out = [], False
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(0.1, start + 120 - time.monotonic()))
        except subprocess.TimeoutExpired:
            timed_out = True
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    if timed_out:
        _broken.append("timed out")
    elif any(p.returncode < 0 for p in procs):
        _broken.append("died on a signal")
    bad = [r for r, p in enumerate(procs) if p.returncode != 0 or f"rank {r} {what} OK" not in outs[r]]
    # (every failing rank's output: the rank that fails first is rarely the one that reports a timeout)
    assert not bad, "\n".join(f"rank {r} (rc {procs[r].returncode}):\n{outs[r][-2000:]}" for r in bad)


def test_engine_ranks(gpu):
    size, key = 3, "r" + uuid.uuid4().hex[:12]
    env = dict(os.environ, MI355X_TIMEOUT_S="60")
    env.pop("MI355X_NB_ORDER", None)
    _run([["engine", key, str(r), str(size), "0"] for r in range(size)], [env] * size, "engine")


@pytest.mark.parametrize("order", [0, 1])
def test_component_processes(gpu, order):
    size, key = 3, uuid.uuid4().hex[:10]
    env = dict(os.environ, MI355X_TIMEOUT_S="60", OMPI_COMM_WORLD_SIZE=str(size), OMPI_COMM_WORLD_LOCAL_SIZE=str(size),
               OMPI_MCA_ess_base_jobid=key, OMPI_MCA_coll_mi355x_nb_order=str(order))
    _run([["component", str(r), str(size), key] for r in range(size)],
         [dict(env, OMPI_COMM_WORLD_LOCAL_RANK=str(r), OMPI_COMM_WORLD_RANK=str(r)) for r in range(size)], "component")
