"""One rank of tests/test_reduction_paths_gpu.py: which path each reduction entry point of coll/mi355x
takes, through the mini harness with the host module installed below the component.

  reduction_paths_worker.py <rank> <size> <key> <mixed>

One loop over {allreduce, reduce (root = 2), reduce_scatter_block, reduce_scatter, scan, exscan} x
{blocking, nonblocking} x {not in place, in place (reduce: on the root only)} runs under three buffer
scenarios:
  (a) every rank on device buffers, MPI_SUM over MPI_INT: the engine serves the call;
  (b) rank 0 on host buffers, the others on device (<mixed> = 1 only): the engine serves the call, the
      host rank joins it on device copies;
  (c) a non-commutative user op (inout = 3 * in + inout) on device buffers: the call is staged through
      host memory to the host module, once, and no device pointer reaches that module.
The host module's counter of the slot and mca_coll_mi355x_staged_calls say which path ran; the results
are exact (numpy for MPI_SUM; for the user op the host module's orders: coll/basic's linear order,
libnbc's binomial tree for MPI_Ireduce_scatter, the rank-order chain for the scans).
"""
from __future__ import annotations

import ctypes
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))

COUNT, RCOUNT, RCOUNTS, ROOT = 257, 5, [5, 0, 3], 2   # rank 1 of the vector form receives nothing
SENTINEL, PAD = -9, 4
COLLS = ("allreduce", "reduce", "reduce_scatter_block", "reduce_scatter", "scan", "exscan")
# mini_host_calls ids of the (blocking, nonblocking) slots
HOST_ID = {"allreduce": (0, 6), "reduce": (5, 11), "reduce_scatter_block": (1, 12), "reduce_scatter": (2, 17),
           "scan": (9, 15), "exscan": (10, 16)}


def user(a, b):
    """a op b of the user function: a = in, b = inout (int32, wrapping)"""
    return (a * np.int32(3) + b).astype(np.int32)


def linear(xs):
    """coll/basic's linear order (coll_basic_reduce.c:215-250): acc = x[n-1], then acc = x[i] op acc"""
    acc = xs[-1].copy()
    for x in reversed(xs[:-1]):
        acc = user(x, acc)
    return acc


def binomial(xs, v=0):
    """libnbc's binomial tree to rank 0 (nbc_ireduce.c:229-282): per round own (op) received"""
    out, r = xs[v].copy(), 1
    while v % (1 << r) == 0 and (1 << (r - 1)) < len(xs):
        p = v + (1 << (r - 1))
        if p < len(xs):
            out = user(out, binomial(xs, p))
        r += 1
    return out


def chain(xs):
    """the rank-order chain of the scans: p[k] = p[k-1] op x[k]"""
    out = [xs[0].copy()]
    for x in xs[1:]:
        out.append(user(out[-1], x))
    return out


def main():
    from mini import mini
    rank, size, key, mixed = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    assert size == len(RCOUNTS)
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    m = mini()
    L, pkg = m.lib, m.pkg
    from conftest import load_oracle
    m.install_oracle_base(load_oracle())
    vp, i = ctypes.c_void_p, ctypes.c_int
    P = ctypes.POINTER(vp)
    L.mini_iscan.argtypes = [vp, vp, vp, i, vp, vp, P]
    L.mini_iexscan.argtypes = [vp, vp, vp, i, vp, vp, P]
    L.mini_ireduce_scatter.argtypes = [vp, vp, vp, ctypes.POINTER(i), vp, vp, P]
    L.mini_host_module.restype = vp
    L.mini_host_calls.argtypes = [i]
    L.mini_op_create_user.restype = vp
    L.mini_op_create_user.argtypes = [vp, i]
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    assert ctypes.c_int.in_dll(m.coll, "mca_coll_mi355x_mixed_buffers").value == mixed
    comm = L.mini_comm_create(rank, size, 95)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_host_module())
    assert L.mini_coll_select(comm, comp) == 90
    staged = ctypes.c_ulong.in_dll(m.coll, "mca_coll_mi355x_staged_calls")
    idt = m.dtype_for_slot(pkg.T["INT32"])
    sum_op = m.select_op(pkg.OP["SUM"])
    USER = ctypes.CFUNCTYPE(None, vp, vp, ctypes.POINTER(ctypes.c_int), vp)

    @USER
    def user_fn(invec, inoutvec, lenp, dtp):
        n = lenp[0]
        a = np.ctypeslib.as_array(ctypes.cast(invec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b = np.ctypeslib.as_array(ctypes.cast(inoutvec, ctypes.POINTER(ctypes.c_int32)), (n,))
        b[:] = a * np.int32(3) + b

    user_op = L.mini_op_create_user(ctypes.cast(user_fn, vp).value, 0)

    def put(a, on_host):
        if on_host:
            h = np.ascontiguousarray(a).copy()
            return h, h.ctypes.data, (lambda: h.copy())
        d = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        return d, d.data_ptr(), (lambda: d.cpu().numpy().view(a.dtype).copy())

    # (input elements, output elements, first output element within the reduced vector) of this rank
    shape = {c: (COUNT, COUNT, 0) for c in COLLS}
    shape["reduce_scatter_block"] = (RCOUNT * size, RCOUNT, RCOUNT * rank)
    shape["reduce_scatter"] = (sum(RCOUNTS), RCOUNTS[rank], sum(RCOUNTS[:rank]))
    xs = {c: [(np.arange(shape[c][0], dtype=np.int32) * (r + 2) + 11 * r).astype(np.int32) for r in range(size)]
          for c in COLLS}
    # what each rank's rbuf holds afterwards (None: left as it was); computed once
    want = {}
    for c in COLLS:
        n_in, n_out, lo = shape[c]
        total = np.sum(xs[c], axis=0, dtype=np.int32)
        for nb in (0, 1):
            if c in ("scan", "exscan"):
                pre_sum, pre_user = np.cumsum(xs[c], axis=0, dtype=np.int32), chain(xs[c])
                k = rank - (c == "exscan")
                want[c, nb, "sum"], want[c, nb, "user"] = (None, None) if k < 0 else (pre_sum[k], pre_user[k])
            else:
                full = binomial(xs[c]) if (c, nb) == ("reduce_scatter", 1) else linear(xs[c])
                sig = c != "reduce" or rank == ROOT
                want[c, nb, "sum"] = total[lo:lo + n_out] if sig else None
                want[c, nb, "user"] = full[lo:lo + n_out] if sig else None
    q = vp()

    def call(c, nb, sp, rp, op):
        if c == "reduce_scatter":
            arr = (ctypes.c_int * size)(*RCOUNTS)
            rc = L.mini_ireduce_scatter(comm, sp, rp, arr, idt, op, ctypes.byref(q)) if nb else \
                L.mini_reduce_scatter(comm, sp, rp, arr, idt, op)
        elif c == "reduce":
            rc = L.mini_ireduce(comm, sp, rp, COUNT, idt, op, ROOT, ctypes.byref(q)) if nb else \
                L.mini_reduce(comm, sp, rp, COUNT, idt, op, ROOT)
        else:
            n = RCOUNT if c == "reduce_scatter_block" else COUNT
            fn = getattr(L, "mini_" + ("i" if nb else "") + c)
            rc = fn(comm, sp, rp, n, idt, op, ctypes.byref(q)) if nb else fn(comm, sp, rp, n, idt, op)
        assert rc == 0, (c, nb, rc)
        if nb:
            assert L.mini_wait(ctypes.byref(q)) == 0, (c, nb)

    def scenario(name, on_host, op, kind):
        for c in COLLS:
            n_in, n_out, _ = shape[c]
            for nb in (0, 1):
                for inplace in (False, True):
                    what = f"({name}) {'i' if nb else ''}{c} inplace={inplace}"
                    ip = inplace and (c != "reduce" or rank == ROOT)   # MPI_IN_PLACE: the root's only
                    x = xs[c][rank]
                    before = x if ip else np.full(n_out + PAD, SENTINEL, np.int32)
                    keep_s, sp, _ = (None, 1, None) if ip else put(x, on_host)
                    keep_r, rp, read = put(before, on_host)
                    torch.cuda.synchronize()
                    calls0, staged0 = L.mini_host_calls(HOST_ID[c][nb]), staged.value
                    call(c, nb, sp, rp, op)
                    got, w = read(), want[c, nb, kind]
                    if w is None:   # a non-root's rbuf, rank 0's rbuf of an exscan: untouched
                        assert np.array_equal(got, before), what + ": rbuf is not significant here, yet written"
                    else:
                        assert np.array_equal(got[:n_out], w), what
                        # (in place the rest of rbuf is input, which the call may use as work space)
                        assert ip or np.array_equal(got[n_out:], before[n_out:]), what + ": wrote past the result"
                    moved = (L.mini_host_calls(HOST_ID[c][nb]) - calls0, staged.value - staged0)
                    assert moved == ((1, 1) if kind == "user" else (0, 0)), (what, moved)

    scenario("a", False, sum_op, "sum")
    if mixed:
        # one device-only call first, so that this window of the buffer-kind vote has seen device use
        x, px, _ = put(xs["allreduce"][rank], False)
        y, py, _ = put(np.zeros(COUNT, np.int32), False)
        torch.cuda.synchronize()
        assert L.mini_allreduce(comm, px, py, COUNT, idt, sum_op) == 0
        scenario("b", rank == 0, sum_op, "sum")
    scenario("c", False, user_op, "user")
    assert L.mini_device_hits() == 0, "a device pointer reached the host module"
    L.mini_comm_destroy(comm)
    L.mini_op_destroy(sum_op)
    L.mini_op_destroy(user_op)
    print(f"rank {rank} paths OK", flush=True)


if __name__ == "__main__":
    main()
