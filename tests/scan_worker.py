"""One rank of tests/test_scan_part_ipc_gpu.py: the partitioned scan flow between processes.

  scan_worker.py engine <key> <rank> <size> <device>   the engine's C ABI, MI355X_SCAN_PART_MIN_BYTES=1
  scan_worker.py component <rank> <size> <key>         coll/mi355x through the mini harness,
                                                       OMPI_MCA_coll_mi355x_scan_part_min_bytes=1

Every rank builds every rank's input from the same seeds, evaluates the reference chain on the CPU
(oracle_scan: coll/basic's; nbc_scan_oracle: libnbc's) and compares its own result bit for bit.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))
import nbc_oracle as nbc  # noqa: E402
import nbc_scan_oracle as nbs  # noqa: E402
import opdata  # noqa: E402

BASE = 60_001       # elements of the first calls: the scratch is allocated at its smallest size
GROWN = 64 * BASE   # ... of the call after which the owners' scratch has been reallocated


def _inputs(tname, count, size, salt):
    if tname == "FLOAT":
        return [np.random.default_rng(9000 + 97 * salt + r).standard_normal(count).astype(np.float32) for r in range(size)]
    return [nbc.tie_nan_pairs(opdata.dtype_of(tname), count, 97 * salt + r) for r in range(size)]


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _basic(oracle, exclusive, ty, op, xs, before):
    want = [b.copy() for b in before]
    assert oracle.oracle_scan(int(exclusive), len(xs), len(xs[0]), ty, op, _ptrs(xs), _ptrs(want)) == 0
    return want


def engine_main():
    from conftest import load_oracle, load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg, oracle = load_pkg(), load_oracle()
    comm = pkg.Comm.create(key, rank, size, dev)
    assert comm.get("SCAN_PART_MIN_BYTES") == 1, "MI355X_SCAN_PART_MIN_BYTES sets the knob at creation"

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def host_of(t, like):
        return t[: like.nbytes].cpu().numpy().view(like.dtype).copy()

    def check(opname, tname, count, salt, libnbc=False):
        """scan and exscan, blocking and nonblocking, in place and not, of one set of inputs"""
        op, ty = pkg.OP[opname], pkg.T[tname]
        xs = _inputs(tname, count, size, salt)
        fill = _inputs(tname, count, 1, 555)[0]
        dx = dev_of(xs[rank])
        for exclusive in (False, True):
            for inplace in (False, True):
                before = [x if inplace else fill for x in xs]
                for nonblocking in (False, True):
                    if libnbc and nonblocking:
                        want = nbs.iexscan(oracle, op, ty, xs, before, inplace) if exclusive else \
                            nbs.iscan(oracle, op, ty, xs, inplace)
                    else:
                        want = _basic(oracle, exclusive, ty, op, xs, before)
                    dr = dev_of(before[rank])
                    torch.cuda.synchronize()
                    sp = None if inplace else dx.data_ptr()
                    if nonblocking:
                        (comm.iexscan if exclusive else comm.iscan)(sp, dr.data_ptr(), count, ty, op).wait()
                    else:
                        (comm.exscan if exclusive else comm.scan)(sp, dr.data_ptr(), count, ty, op)
                    what = f"{tname} count={count} exclusive={exclusive} inplace={inplace} nonblocking={nonblocking}"
                    assert comm.last_algorithm() == 2, what
                    got = host_of(dr, xs[rank])
                    if exclusive and rank == 0:
                        assert got.tobytes() == before[0].tobytes(), what + ": rank 0's rbuf was written"
                    else:
                        opdata.assert_same(tname, opname, got, want[rank], what)

    check("SUM", "FLOAT", BASE, 1)
    check("SUM", "FLOAT", GROWN, 2)     # the owners' scratch regrows: the peers map the new allocation
    check("SUM", "FLOAT", BASE, 3)      # ... and keep using it
    check("SUM", "FLOAT", 2, 4)         # the last block is empty
    comm.barrier()
    comm.set("NB_ORDER", 1)
    comm.barrier()
    check("MAXLOC", "FLOAT_INT", 4099, 5, libnbc=True)
    # the knob at 0: the chain, the same bytes
    comm.barrier()
    comm.set("SCAN_PART_MIN_BYTES", 0)
    comm.set("NB_ORDER", 0)
    comm.barrier()
    op, ty = pkg.OP["SUM"], pkg.T["FLOAT"]
    xs = _inputs("FLOAT", BASE, size, 1)
    want = _basic(oracle, False, ty, op, xs, [np.zeros_like(x) for x in xs])
    dx, dr = dev_of(xs[rank]), dev_of(np.zeros_like(xs[rank]))
    torch.cuda.synchronize()
    comm.scan(dx.data_ptr(), dr.data_ptr(), BASE, ty, op)
    assert comm.last_algorithm() == 1
    opdata.assert_same("FLOAT", "SUM", host_of(dr, xs[rank]), want[rank], "the chain")
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    from conftest import load_oracle
    from mini import mini
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    assert os.environ.get("OMPI_MCA_coll_mi355x_scan_part_min_bytes") == "1"
    m = mini()
    L, pkg = m.lib, m.pkg
    oracle = load_oracle()
    m.install_oracle_base(oracle)
    vp, i = ctypes.c_void_p, ctypes.c_int
    P = ctypes.POINTER(vp)
    L.mini_iscan.argtypes = [vp, vp, vp, i, vp, vp, P]
    L.mini_iexscan.argtypes = [vp, vp, vp, i, vp, vp, P]
    L.mini_host_module.restype = vp
    L.mini_host_calls.argtypes = [i]
    L.mini_op_create_user.restype = vp
    L.mini_op_create_user.argtypes = [vp, i]
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    comm = L.mini_comm_create(rank, size, 91)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_host_module())
    assert L.mini_coll_select(comm, comp) == 90
    assert L.mini_comm_fn(comm, 20) == m.addr(m.coll, "mca_coll_mi355x_iscan")
    assert L.mini_comm_fn(comm, 21) == m.addr(m.coll, "mca_coll_mi355x_iexscan")
    m.coll.mca_coll_mi355x_engine_of.restype = vp
    m.coll.mca_coll_mi355x_engine_of.argtypes = [vp]
    eng = pkg.Comm(m.coll.mca_coll_mi355x_engine_of(comm))
    assert eng.get("SCAN_PART_MIN_BYTES") == 1, "coll_mi355x_scan_part_min_bytes reaches the engine"
    code, slot = pkg.OP["SUM"], pkg.T["FLOAT"]
    dt, op = m.dtype_for_slot(slot), m.select_op(code)
    q = vp()

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def run(fn, sp, rp, count, dtype=dt, mpi_op=None):
        assert fn(comm, sp, rp, count, dtype, mpi_op or op, ctypes.byref(q)) == 0
        assert L.mini_wait(ctypes.byref(q)) == 0

    # MPI_Iscan / MPI_Iexscan on device buffers, before and after the scratch has regrown
    for count, salt in ((BASE, 21), (GROWN, 22), (BASE, 23)):
        xs = _inputs("FLOAT", count, size, salt)
        fill = _inputs("FLOAT", count, 1, 556)[0]
        dx = dev_of(xs[rank])
        for exclusive, fn in ((False, L.mini_iscan), (True, L.mini_iexscan)):
            want = _basic(oracle, exclusive, slot, code, xs, [fill] * size)
            dr = dev_of(fill)
            torch.cuda.synchronize()
            run(fn, dx.data_ptr(), dr.data_ptr(), count)
            assert eng.last_algorithm() == 2
            got = dr.cpu().numpy().view(np.float32)
            # (rank 0 of the exclusive form: want[0] is the fill, untouched)
            opdata.assert_same("FLOAT", "SUM", got, want[rank], f"device buffers count={count} exclusive={exclusive}")
            di = dev_of(xs[rank])      # MPI_IN_PLACE
            torch.cuda.synchronize()
            run(fn, 1, di.data_ptr(), count)
            wi = _basic(oracle, exclusive, slot, code, xs, xs)
            opdata.assert_same("FLOAT", "SUM", di.cpu().numpy().view(np.float32), wi[rank],
                               f"device buffers in place count={count} exclusive={exclusive}")
    # host buffers on every rank (coll_mi355x_mixed_buffers): the ranks join the engine on device copies
    count = 4099
    xs = _inputs("FLOAT", count, size, 24)
    fill = _inputs("FLOAT", count, 1, 557)[0]
    for exclusive, fn in ((False, L.mini_iscan), (True, L.mini_iexscan)):
        want = _basic(oracle, exclusive, slot, code, xs, [fill] * size)
        hs, hr = xs[rank].copy(), fill.copy()
        run(fn, hs.ctypes.data, hr.ctypes.data, count)
        opdata.assert_same("FLOAT", "SUM", hr, want[rank], f"host buffers exclusive={exclusive}")
    assert (L.mini_host_calls(15), L.mini_host_calls(16)) == (0, 0), "the engine served every call so far"
    # a user-defined op: declined, staged through the host to the lower-priority module
    USER = ctypes.CFUNCTYPE(None, vp, vp, ctypes.POINTER(ctypes.c_int), vp)

    @USER
    def user_fn(invec, inoutvec, lenp, dtp):
        n = lenp[0]
        a = np.ctypeslib.as_array(ctypes.cast(invec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b = np.ctypeslib.as_array(ctypes.cast(inoutvec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b[:] = a * np.int32(3) + b

    uop = L.mini_op_create_user(ctypes.cast(user_fn, vp).value, 0)
    idt = m.dtype_for_slot(pkg.T["INT32"])
    count = 7001
    ys = [(np.arange(count, dtype=np.int32) * (r + 2) + 11 * r).astype(np.int32) for r in range(size)]
    chain = [ys[0].copy()]   # ompi_op_reduce(op, partial, x_k): x_k = partial op x_k
    for k in range(1, size):
        chain.append((chain[-1] * np.int32(3) + ys[k]).astype(np.int32))
    dy = dev_of(ys[rank])
    marks = np.full(count, -7, dtype=np.int32)
    for exclusive, fn, which in ((False, L.mini_iscan, 15), (True, L.mini_iexscan, 16)):
        do = dev_of(marks)
        torch.cuda.synchronize()
        run(fn, dy.data_ptr(), do.data_ptr(), count, idt, uop)
        want = (marks if rank == 0 else chain[rank - 1]) if exclusive else chain[rank]
        assert np.array_equal(do.cpu().numpy().view(np.int32), want), f"user op exclusive={exclusive}"
        assert L.mini_host_calls(which) == 1, "the user-op call went to the lower-priority module, once"
    assert L.mini_device_hits() == 0, "a device pointer reached the host module"
    L.mini_comm_destroy(comm)
    L.mini_op_destroy(op)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
