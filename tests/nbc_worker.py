"""One rank of tests/test_nbc_ipc_gpu.py: coll/libnbc's operand order between processes.

  nbc_worker.py engine <key> <rank> <size> <device>   the engine's C ABI, MI355X_NB_ORDER=1
  nbc_worker.py component <rank> <size> <key>         coll/mi355x through the mini harness,
                                                      OMPI_MCA_coll_mi355x_nb_order=1

Every rank builds every rank's input from the same seeds, runs the message-passing simulation of
libnbc's schedule (nbc_oracle.py) and compares its own result bit for bit.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))
import nbc_oracle as nbc  # noqa: E402
import opdata  # noqa: E402


def _inputs(tname, count, size, salt):
    if tname == "FLOAT":
        return [np.random.default_rng(7000 + 97 * salt + r).standard_normal(count).astype(np.float32) for r in range(size)]
    return [nbc.tie_nan_pairs(opdata.dtype_of(tname), count, 97 * salt + r) for r in range(size)]


def engine_main():
    from conftest import load_oracle, load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg, oracle = load_pkg(), load_oracle()
    comm = pkg.Comm.create(key, rank, size, dev)
    assert comm.get("NB_ORDER") == 1, "MI355X_NB_ORDER=1 sets the knob at creation"

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def host_of(t, like, n=None):
        n = len(like) if n is None else n
        return t[: n * like.dtype.itemsize].cpu().numpy().view(like.dtype).copy()

    def iallreduce(opname, tname, nbytes, salt, want_alg):
        op, ty = pkg.OP[opname], pkg.T[tname]
        esz = pkg.type_size(ty)
        count = nbytes // esz
        xs = _inputs(tname, count, size, salt)
        want, alg = nbc.iallreduce(oracle, op, ty, xs, esz)
        assert alg == want_alg, (nbytes, alg)
        dx = dev_of(xs[rank])
        dr = torch.zeros_like(dx)
        torch.cuda.synchronize()
        comm.iallreduce(dx.data_ptr(), dr.data_ptr(), count, ty, op).wait()
        assert comm.last_algorithm() == alg, (nbytes, comm.last_algorithm())
        opdata.assert_same(tname, opname, host_of(dr, want[rank]), want[rank], f"iallreduce {nbytes} B rank {rank}")

    op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
    if size == 4:
        # (sizes of the engine's resident-service, service-pull, one-phase and two-phase / pipelined
        # ranges: a libnbc-ordered call takes none of the first two and never the pipelined kernel)
        iallreduce("SUM", "FLOAT", 1 << 10, 1, nbc.BINOMIAL)   # (the first call: the device setup)
        before = comm.get("PIPE_CALLS"), comm.get("SVC_CALLS")
        iallreduce("SUM", "FLOAT", 1 << 10, 1, nbc.BINOMIAL)
        iallreduce("SUM", "FLOAT", 96 << 10, 2, nbc.RING)
        iallreduce("SUM", "FLOAT", 512 << 10, 3, nbc.RING)
        iallreduce("SUM", "FLOAT", 4 << 20, 4, nbc.RING)
        assert (comm.get("PIPE_CALLS"), comm.get("SVC_CALLS")) == before
        count = (96 << 10) // 4
        xs = _inputs("FLOAT", count, size, 5)
        dx = dev_of(xs[rank])
        for root in (0, 2):
            want, alg = nbc.ireduce(oracle, op, ty, xs, 4, root)
            assert alg == nbc.CHAIN
            dr = torch.zeros_like(dx)
            torch.cuda.synchronize()
            comm.ireduce(dx.data_ptr(), dr.data_ptr() if rank == root else None, count, ty, op, root).wait()
            assert comm.last_algorithm() == nbc.CHAIN
            if rank == root:
                opdata.assert_same("FLOAT", "SUM", host_of(dr, want), want, f"ireduce chain root {root}")
        rcount = 300
        xs = _inputs("FLOAT", rcount * size, size, 6)
        want, _ = nbc.ireduce_scatter_block(oracle, op, ty, xs, rcount)
        dx = dev_of(xs[rank])
        dr = torch.zeros(rcount * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        comm.ireduce_scatter_block(dx.data_ptr(), dr.data_ptr(), rcount, ty, op).wait()
        assert comm.last_algorithm() == nbc.BINOMIAL
        opdata.assert_same("FLOAT", "SUM", host_of(dr, want[rank]), want[rank], f"ireduce_scatter_block rank {rank}")
        iallreduce("MAXLOC", "FLOAT_INT", 1 << 10, 7, nbc.BINOMIAL)
    else:
        iallreduce("SUM", "FLOAT", 1 << 10, 8, nbc.BINOMIAL)
        iallreduce("SUM", "FLOAT", 96 << 10, 9, nbc.BINOMIAL)
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    import coll_worker as cw   # the harness helpers (mini, the oracle loader) as coll_worker.py sets them up
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    assert os.environ.get("OMPI_MCA_coll_mi355x_nb_order") == "1"
    m = cw.mini()
    L, pkg = m.lib, m.pkg
    oracle = cw.load_oracle()
    m.install_oracle_base(oracle)
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    comm = L.mini_comm_create(rank, size, 77)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_stub_module())
    assert L.mini_coll_select(comm, comp) == 90
    m.coll.mca_coll_mi355x_engine_of.restype = ctypes.c_void_p
    m.coll.mca_coll_mi355x_engine_of.argtypes = [ctypes.c_void_p]
    eng = pkg.Comm(m.coll.mca_coll_mi355x_engine_of(comm))
    assert eng.get("NB_ORDER") == 1, "coll_mi355x_nb_order reaches the engine"
    ptrs = lambda arrs: (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])  # noqa: E731
    code, slot = pkg.OP["SUM"], pkg.T["FLOAT"]
    dt, op = m.dtype_for_slot(slot), m.select_op(code)
    count = 16385
    xs = _inputs("FLOAT", count, size, 11)
    want, alg = nbc.iallreduce(oracle, code, slot, xs, 4)
    tuned = [np.zeros_like(xs[0]) for _ in range(size)]
    assert oracle.oracle_allreduce(0, size, count, slot, code, 0, ptrs(xs), ptrs(tuned)) >= 0
    assert len(opdata.mismatches("FLOAT", "SUM", want[rank], tuned[rank])) >= count // 10
    # MPI_Iallreduce on device buffers
    dx = torch.from_numpy(xs[rank].view(np.uint8).copy()).cuda()
    dr = torch.zeros_like(dx)
    torch.cuda.synchronize()
    q = ctypes.c_void_p()
    assert L.mini_iallreduce(comm, dx.data_ptr(), dr.data_ptr(), count, dt, op, ctypes.byref(q)) == 0
    assert L.mini_wait(ctypes.byref(q)) == 0
    opdata.assert_same("FLOAT", "SUM", dr.cpu().numpy().view(np.float32), want[rank], "MPI_Iallreduce, device buffers")
    assert eng.last_algorithm() == alg
    # ... and on host buffers on every rank: the ranks join the engine (nb_host_join), so libnbc's order
    hs, hr = xs[rank].copy(), np.zeros_like(xs[rank])
    assert L.mini_iallreduce(comm, hs.ctypes.data, hr.ctypes.data, count, dt, op, ctypes.byref(q)) == 0
    assert L.mini_wait(ctypes.byref(q)) == 0
    opdata.assert_same("FLOAT", "SUM", hr, want[rank], "MPI_Iallreduce, host buffers")
    assert L.mini_stub_calls(6) == 0, "the all-host call stayed in the engine"
    # the blocking call keeps coll/tuned's order
    db = torch.zeros_like(dx)
    torch.cuda.synchronize()
    assert L.mini_allreduce(comm, dx.data_ptr(), db.data_ptr(), count, dt, op) == 0
    opdata.assert_same("FLOAT", "SUM", db.cpu().numpy().view(np.float32), tuned[rank], "MPI_Allreduce")
    L.mini_comm_destroy(comm)
    L.mini_op_destroy(op)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
