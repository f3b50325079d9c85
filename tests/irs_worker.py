"""One rank of tests/test_irs_ipc_gpu.py: MPI_Ireduce_scatter (vector counts) between processes.

  irs_worker.py engine <key> <rank> <size> <device>   the engine's C ABI, both NB_ORDER values
  irs_worker.py component <rank> <size> <key>         coll/mi355x through the mini harness, with
                                                      OMPI_MCA_coll_mi355x_nb_order 0 or 1

Every rank builds every rank's input from the same seeds, evaluates the order's reference on the CPU
(NB_ORDER 0: coll/tuned's reduce_scatter, the oracle's; 1: libnbc's schedule, tests/nbc_rs_oracle.py)
and compares its own block bit for bit.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))
import nbc_oracle as nbc  # noqa: E402
import nbc_rs_oracle as nrs  # noqa: E402
import opdata  # noqa: E402

BIG = 60_001   # elements per rank of the large vector (off every tile and vector width)


def _inputs(tname, count, size, salt):
    if tname == "FLOAT":
        return [np.random.default_rng(7000 + 89 * salt + r).standard_normal(count).astype(np.float32) for r in range(size)]
    return [nbc.tie_nan_pairs(opdata.dtype_of(tname), count, 89 * salt + r) for r in range(size)]


def _ptrs(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _tuned(oracle, ty, op, xs, rcounts):
    """coll/tuned's fixed decision for the vector: (every rank's block, the algorithm)"""
    n = len(xs)
    vp, i = ctypes.c_void_p, ctypes.c_int
    oracle.oracle_reduce_scatter.argtypes = [i, ctypes.POINTER(i), i, i, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    outs = [np.zeros(max(c, 1), dtype=xs[0].dtype) for c in rcounts]
    alg = oracle.oracle_reduce_scatter(n, (ctypes.c_int * n)(*rcounts), ty, op, _ptrs(xs), _ptrs(outs))
    assert alg > 0
    return [o[:c] for o, c in zip(outs, rcounts)], alg


def _want(oracle, order, ty, op, xs, rcounts, inplace):
    if order:
        return nrs.ireduce_scatter(oracle, op, ty, xs, rcounts, inplace)
    return _tuned(oracle, ty, op, xs, rcounts)


def _vectors(size):
    return (("ragged", nrs.counts_of("ragged", size)), ("holes", nrs.counts_of("holes", size)), ("big", [BIG] * size))


def engine_main():
    from conftest import load_oracle, load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg, oracle = load_pkg(), load_oracle()
    comm = pkg.Comm.create(key, rank, size, dev)

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def check(order, opname, tname, salt):
        op, ty = pkg.OP[opname], pkg.T[tname]
        for vi, (kind, rcounts) in enumerate(_vectors(size)):
            xs = _inputs(tname, sum(rcounts), size, 10 * salt + vi)
            esz, k = xs[0].dtype.itemsize, rcounts[rank]
            dx = dev_of(xs[rank])
            for inplace in (False, True):
                want, alg = _want(oracle, order, ty, op, xs, rcounts, inplace)
                dr = dev_of(xs[rank]) if inplace else torch.full((max(k, 1) * esz,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                # a rank that receives nothing may hand in any rbuf, its sbuf included: it is not in place
                # for that (the ranks must agree on the flow; only NB_ORDER 0 has a flow that depends on it)
                rp = dx.data_ptr() if (k == 0 and not inplace) else dr.data_ptr()
                comm.ireduce_scatter(None if inplace else dx.data_ptr(), rp, rcounts, ty, op).wait()
                what = f"NB_ORDER={order} {opname} {tname} {kind} inplace={inplace}"
                assert comm.last_algorithm() == alg, what
                got = dr[: k * esz].cpu().numpy().view(xs[0].dtype)
                opdata.assert_same(tname, opname, got, want[rank], what)

    check(0, "SUM", "FLOAT", 1)
    comm.barrier()
    comm.set("NB_ORDER", 1)
    comm.barrier()
    check(1, "SUM", "FLOAT", 2)
    check(1, "MAXLOC", "FLOAT_INT", 3)
    comm.barrier()
    comm.set("NB_ORDER", 0)
    comm.barrier()
    check(0, "SUM", "FLOAT", 4)
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    from conftest import load_oracle
    from mini import mini
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    order = int(os.environ["OMPI_MCA_coll_mi355x_nb_order"])
    m = mini()
    L, pkg = m.lib, m.pkg
    oracle = load_oracle()
    m.install_oracle_base(oracle)
    vp, i = ctypes.c_void_p, ctypes.c_int
    P = ctypes.POINTER(vp)
    L.mini_ireduce_scatter.argtypes = [vp, vp, vp, ctypes.POINTER(i), vp, vp, P]
    L.mini_host_module.restype = vp
    L.mini_host_calls.argtypes = [i]
    L.mini_op_create_user.restype = vp
    L.mini_op_create_user.argtypes = [vp, i]
    IRS_FN, IRS_HOST = 22, 17   # mini_comm_fn / mini_host_calls ids of the ireduce_scatter slot
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    comm = L.mini_comm_create(rank, size, 93)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_host_module())
    assert L.mini_coll_select(comm, comp) == 90
    assert L.mini_comm_fn(comm, IRS_FN) == m.addr(m.coll, "mca_coll_mi355x_ireduce_scatter")
    m.coll.mca_coll_mi355x_engine_of.restype = vp
    m.coll.mca_coll_mi355x_engine_of.argtypes = [vp]
    eng = pkg.Comm(m.coll.mca_coll_mi355x_engine_of(comm))
    assert eng.get("NB_ORDER") == order, "coll_mi355x_nb_order reaches the engine"
    code, slot = pkg.OP["SUM"], pkg.T["FLOAT"]
    dt, op = m.dtype_for_slot(slot), m.select_op(code)
    q = vp()

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    def run(sp, rp, rcounts, dtype=dt, mpi_op=None):
        arr = (ctypes.c_int * size)(*rcounts)
        assert L.mini_ireduce_scatter(comm, sp, rp, arr, dtype, mpi_op or op, ctypes.byref(q)) == 0
        for j in range(size):   # MPI lets the caller reuse its array once the call has returned
            arr[j] = -1
        assert L.mini_wait(ctypes.byref(q)) == 0

    for vi, kind in enumerate(("ragged", "holes")):
        rcounts = nrs.counts_of(kind, size)
        k = rcounts[rank]
        xs = _inputs("FLOAT", sum(rcounts), size, 30 + vi)
        # device buffers, not in place and in place (MPI_IN_PLACE is (void *)1)
        want, alg = _want(oracle, order, slot, code, xs, rcounts, False)
        dx, dr = dev_of(xs[rank]), torch.zeros(max(k, 1) * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        run(dx.data_ptr(), dr.data_ptr(), rcounts)
        assert eng.last_algorithm() == alg
        opdata.assert_same("FLOAT", "SUM", dr[: 4 * k].cpu().numpy().view(np.float32), want[rank], f"device buffers {kind}")
        wi, _ = _want(oracle, order, slot, code, xs, rcounts, True)
        di = dev_of(xs[rank])
        torch.cuda.synchronize()
        run(1, di.data_ptr(), rcounts)
        opdata.assert_same("FLOAT", "SUM", di[: 4 * k].cpu().numpy().view(np.float32), wi[rank], f"device buffers in place {kind}")
        # host buffers on every rank (coll_mi355x_mixed_buffers): the ranks join the engine on device
        # copies (holes: a rank that receives nothing still stages its input and takes part)
        hs, hr = xs[rank].copy(), np.full(max(k, 1), -3.0, dtype=np.float32)
        run(hs.ctypes.data, hr.ctypes.data, rcounts)
        opdata.assert_same("FLOAT", "SUM", hr[:k], want[rank], f"host buffers {kind}")
        assert (hr[k:] == -3.0).all(), f"host buffers {kind}: wrote past the block"
        hi = xs[rank].copy()
        run(1, hi.ctypes.data, rcounts)
        opdata.assert_same("FLOAT", "SUM", hi[:k], wi[rank], f"host buffers in place {kind}")
    assert L.mini_host_calls(IRS_HOST) == 0, "the engine served every call so far"
    # a user-defined op: declined, staged through the host to the lower-priority module.  That module's
    # h_irs stands in for coll/libnbc, the slot's owner in the reference, and reduces in libnbc's order
    # whatever coll_mi355x_nb_order is (the variable orders the engine, not the module below it): the
    # binomial tree to rank 0, every step target = own (op) received, i.e. the user function called
    # with in = own and inout = a copy of the received piece.
    USER = ctypes.CFUNCTYPE(None, vp, vp, ctypes.POINTER(ctypes.c_int), vp)

    @USER
    def user_fn(invec, inoutvec, lenp, dtp):
        n = lenp[0]
        a = np.ctypeslib.as_array(ctypes.cast(invec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b = np.ctypeslib.as_array(ctypes.cast(inoutvec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b[:] = a * np.int32(3) + b

    uop = L.mini_op_create_user(ctypes.cast(user_fn, vp).value, 0)
    idt = m.dtype_for_slot(pkg.T["INT32"])
    rcounts = nrs.counts_of("ragged", size)
    total, k = sum(rcounts), rcounts[rank]
    ys = [(np.arange(total, dtype=np.int32) * (r + 2) + 11 * r).astype(np.int32) for r in range(size)]

    class UserOracle:   # the user function as nbc_oracle.Sim's 3-buff loop: target = in1 * 3 + in2
        @staticmethod
        def oracle_op_3buff(_op, _ty, in1, in2, out, cnt):
            v = [np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_int32)), (cnt,)) for p in (in1, in2, out)]
            v[2][:] = v[0] * np.int32(3) + v[1]

    want = nrs.ireduce_scatter(UserOracle, 0, 0, ys, rcounts)[0][rank]   # libnbc's schedule, simulated
    dy = dev_of(ys[rank])
    do = dev_of(np.full(k, -7, dtype=np.int32))
    torch.cuda.synchronize()
    run(dy.data_ptr(), do.data_ptr(), rcounts, idt, uop)
    assert np.array_equal(do.cpu().numpy().view(np.int32), want), "user op"
    assert L.mini_host_calls(IRS_HOST) == 1, "the user-op call went to the lower-priority module, once"
    assert L.mini_device_hits() == 0, "a device pointer reached the host module"
    L.mini_comm_destroy(comm)
    L.mini_op_destroy(op)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
