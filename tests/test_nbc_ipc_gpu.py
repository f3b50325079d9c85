"""coll/libnbc's operand order between processes (tests/nbc_worker.py): the engine's C ABI under
MI355X_NB_ORDER=1 at sizes in each of the engine's flow ranges, and the MCA component under
coll_mi355x_nb_order=1 (device buffers, all-host buffers that join the engine, and the blocking
call, which keeps coll/tuned's order).  Every result is bit-exact against the simulation of
libnbc's schedules."""
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
_broken = []   # a worker timed out or died on a signal: the GPU is left alone for the rest of the module


def _run(argvs, envs, what):
    """the workers under ONE 120 s limit; every rank must print 'rank <r> <what> OK'"""
    if _broken:
        pytest.skip(f"an earlier worker of this module {_broken[0]}")
    procs = [subprocess.Popen([sys.executable, str(HERE / "nbc_worker.py")] + a, env=e, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for a, e in zip(argvs, envs)]
    deadline = time.monotonic() + 120
    outs, timed_out = [], False
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(0.1, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            timed_out = True
            p.kill()
            out, _ = p.communicate()
        outs.append(out)
    if timed_out:
        _broken.append("timed out")
    elif any(p.returncode < 0 for p in procs):
        _broken.append("died on a signal")
    for r, p in enumerate(procs):
        assert p.returncode == 0 and f"rank {r} {what} OK" in outs[r], f"rank {r} (rc {p.returncode}):\n{outs[r][-3000:]}"


@pytest.mark.parametrize("size", [4, 3])
def test_engine_ranks(gpu, size):
    """4 ranks: Iallreduce fp32 SUM at 1 KiB (binomial), 96 KiB, 512 KiB and 4 MiB (ring); Ireduce
    96 KiB (chain) to roots 0 and 2; Ireduce_scatter_block; MAXLOC on ties and NaNs.  3 ranks: 1 KiB
    and 96 KiB, both binomial."""
    key = "n" + uuid.uuid4().hex[:12]
    ndev = gpu.cuda.device_count()
    env = dict(os.environ, MI355X_TIMEOUT_S="60", MI355X_NB_ORDER="1")
    _run([["engine", key, str(r), str(size), str(r % ndev)] for r in range(size)], [env] * size, "engine")


def test_component_processes(gpu):
    """3 processes through the harness with OMPI_MCA_coll_mi355x_nb_order=1"""
    size, key = 3, uuid.uuid4().hex[:10]
    env = dict(os.environ, MI355X_TIMEOUT_S="60", OMPI_COMM_WORLD_SIZE=str(size), OMPI_COMM_WORLD_LOCAL_SIZE=str(size),
               OMPI_MCA_ess_base_jobid=key, OMPI_MCA_coll_mi355x_nb_order="1")
    _run([["component", str(r), str(size), key] for r in range(size)],
         [dict(env, OMPI_COMM_WORLD_LOCAL_RANK=str(r), OMPI_COMM_WORLD_RANK=str(r)) for r in range(size)], "component")
