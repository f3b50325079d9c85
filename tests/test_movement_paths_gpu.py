"""The path table of coll/mi355x's data-movement entry points (tests/movement_paths_worker.py), 3
processes on one GPU through the mini harness with the host module below the component: allgather,
bcast, gather(v), scatter(v), allgatherv and alltoall(v), in place and not, and iallgather / ibcast.
Device buffers and a rank on host buffers among device ranks are served by the engine (no counter of
the host module or the stub moves, nor mca_coll_mi355x_staged_calls); once the buffer-kind vote says
host, every call goes to the previous owner, each device rank staging its buffers exactly once, and a
call the previous owner fails copies nothing back.  Bad arguments reach the previous owner without a
vote; a negative displacement is refused before anything is staged.  With coll_mi355x_mixed_buffers =
0 a host side sends iallgather / ibcast to the host module's nonblocking slots.  Every result is exact;
gaps, padding and non-significant buffers keep their sentinel."""
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
    procs = [subprocess.Popen([sys.executable, str(HERE / "movement_paths_worker.py")] + a, env=e,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for a, e in zip(argvs, envs)]
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


@pytest.mark.parametrize("mixed", [1, 0])
def test_movement_paths(gpu, mixed):
    size, key = 3, uuid.uuid4().hex[:10]
    env = dict(os.environ, MI355X_TIMEOUT_S="60", OMPI_COMM_WORLD_SIZE=str(size), OMPI_COMM_WORLD_LOCAL_SIZE=str(size),
               OMPI_MCA_ess_base_jobid=key)
    env.pop("OMPI_MCA_coll_mi355x_nb_order", None)
    if mixed:
        env.pop("OMPI_MCA_coll_mi355x_mixed_buffers", None)   # the default
    else:
        env["OMPI_MCA_coll_mi355x_mixed_buffers"] = "0"
    _run([[str(r), str(size), key, str(mixed)] for r in range(size)],
         [dict(env, OMPI_COMM_WORLD_LOCAL_RANK=str(r), OMPI_COMM_WORLD_RANK=str(r)) for r in range(size)], "paths")
