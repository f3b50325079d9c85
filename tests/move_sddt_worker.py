"""One rank of tests/test_move_sddt_ipc_gpu.py: the movement collectives pulling straight out of a
derived send datatype, between processes.

  move_sddt_worker.py engine <key> <rank> <size> <device>   mi355x_alltoallv_ddt2 / mi355x_gatherv_ddt2
  move_sddt_worker.py component <rank> <size> <key>         MPI_Alltoall through coll/mi355x (mini harness)

engine: ranks 0 and 2 send through a layout (vector(9, 64, 128) of floats; columns of doubles resized to
one element, so the pieces interleave in the sender's memory) and publish it, rank 1 calls the PLAIN
form with dense bytes in the same collective.  Every rank builds every rank's bytes from the same seeds
and compares its own result byte for byte with the numpy model of tests/move_ddt_model.py.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))
import move_ddt_model as mdl  # noqa: E402

G, POISON, FILL = mdl.GUARD, mdl.POISON, 0x5A


def send_side(name, cnt):
    """layout, byte displacement of every piece, bytes the send buffer spans"""
    if name == "col8":
        rows, ncols = 33, sum(cnt) + 1
        first = np.concatenate([[0], np.cumsum(cnt[:-1])])
        return mdl.column(rows, ncols), [int(c) * 8 for c in first], rows * ncols * 8
    lay, displs, at = mdl.vec9(), [], 0
    for c in cnt:
        displs.append(at)
        at += lay.span(c) + 48
    return lay, displs, at


def engine_main():
    from conftest import load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg = load_pkg()
    comm = pkg.Comm.create(key, rank, size, dev)
    assert comm.get("MOVE_SEND_MIN_RUN") == 8, "MI355X_MOVE_SEND_MIN_RUN sets the knob at creation"
    plain = rank == 1
    direct = 0

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def offs(nbytes):
        return [int(v) for v in np.concatenate([[0], np.cumsum(nbytes[:-1])])]

    for name in ("vec9", "col8"):
        # ---- alltoallv: sender q sends counts[q][r] instances of its layout to r; every receiver takes dense bytes
        counts = [[1 + (2 * q + r) % 4 for r in range(size)] for q in range(size)]
        lay, sdis, total = send_side(name, counts[rank])
        size1 = lay.size
        data = [[mdl.payload(7000 + 10 * q + r, counts[q][r] * size1) for r in range(size)] for q in range(size)]
        sent = [counts[rank][r] * size1 for r in range(size)]
        caps = [counts[q][rank] * size1 for q in range(size)]
        rbuf = torch.full((sum(caps) + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
        want = np.full(rbuf.numel(), POISON, dtype=np.uint8)
        for q in range(size):
            want[G + offs(caps)[q]:G + offs(caps)[q] + caps[q]] = data[q][rank]
        if plain:
            host = np.concatenate(data[rank])
            sbuf = dev_of(host)
            torch.cuda.synchronize()
            comm.alltoallv(sbuf.data_ptr(), sent, offs(sent), rbuf.data_ptr() + G, caps, offs(caps))
        else:
            host = np.full(total + 2 * G, FILL, dtype=np.uint8)
            for r in range(size):
                host[G + sdis[r] + lay.offsets(sent[r])] = data[rank][r]
            sbuf = dev_of(host)
            torch.cuda.synchronize()
            comm.alltoallv_ddt2(sbuf.data_ptr() + G, lay.ddt(pkg), counts[rank], sdis, rbuf.data_ptr() + G, None, caps,
                                offs(caps))
            direct += 1
        assert np.array_equal(rbuf.cpu().numpy(), want), f"alltoallv out of {name}"
        assert np.array_equal(sbuf.cpu().numpy(), host), f"alltoallv out of {name}: the send buffer changed"
        comm.barrier()
        # ---- gatherv to every root in turn: the root takes dense bytes
        for root in range(size):
            cnt = counts[root]
            gl, gd, gt = send_side(name, [cnt[rank]])
            gdata = [mdl.payload(8000 + 10 * root + q, cnt[q] * gl.size) for q in range(size)]
            gcap = [len(d) for d in gdata]
            am_root = rank == root
            gr = torch.full((sum(gcap) + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
            gw = np.full(gr.numel(), POISON, dtype=np.uint8)
            if am_root:
                for q in range(size):
                    gw[G + offs(gcap)[q]:G + offs(gcap)[q] + gcap[q]] = gdata[q]
            rargs = (gr.data_ptr() + G, gcap, offs(gcap)) if am_root else (None, None, None)
            if plain:
                gs = dev_of(gdata[rank])
                torch.cuda.synchronize()
                comm.gatherv(gs.data_ptr(), gcap[rank], rargs[0], rargs[1], rargs[2], root)
            else:
                gh = np.full(gt + 2 * G, FILL, dtype=np.uint8)
                gh[G + gl.offsets(gcap[rank])] = gdata[rank]
                gs = dev_of(gh)
                torch.cuda.synchronize()
                comm.gatherv_ddt2(gs.data_ptr() + G, gl.ddt(pkg), cnt[rank], rargs[0], None, rargs[1], rargs[2], root)
                direct += 1
            assert np.array_equal(gr.cpu().numpy(), gw), f"gatherv out of {name} at root {root}"
            comm.barrier()
    assert comm.get("MOVE_SEND_DIRECT") == direct, (comm.get("MOVE_SEND_DIRECT"), direct)
    assert (direct == 0) == plain
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    """MPI_Alltoall of a 301 x size matrix of doubles, the send side a column type (vector(301, 1, size,
    MPI_DOUBLE) resized to one element): the component hands the layout to the engine, which publishes it;
    then the column type on both sides -- the block transpose, nothing packed, nothing unpacked"""
    from ddtcases import opal_strided_elems
    from mini import mini
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    min_run = int(os.environ["OMPI_MCA_coll_mi355x_move_send_min_run"])
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    m = mini()
    L, pkg = m.lib, m.pkg
    vp = ctypes.c_void_p
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    comm = L.mini_comm_create(rank, size, 94)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_stub_module())
    assert L.mini_coll_select(comm, comp) == 90
    m.coll.mca_coll_mi355x_engine_of.restype = vp
    m.coll.mca_coll_mi355x_engine_of.argtypes = [vp]
    eng = pkg.Comm(m.coll.mca_coll_mi355x_engine_of(comm))
    assert eng.get("MOVE_SEND_MIN_RUN") == min_run, "coll_mi355x_move_send_min_run reaches the engine"
    n = 301
    dbl = m.dtype_for_slot(pkg.T["DOUBLE"])
    OPAL_FLOAT8 = 16   # opal_datatype_internal.h:107-131 (OPAL_DATATYPE_FLOAT8)
    desc, used, tsize, _, true_ub = opal_strided_elems(n, OPAL_FLOAT8, 8, 8 * size)
    col = L.mini_datatype_create_raw(desc, used, tsize, 0, 8, 0, true_ub, 0)   # MPI_Type_create_resized(.., 0, 8)
    # rank q's matrix: column r goes to rank r
    mats = [np.random.default_rng(9100 + q).standard_normal((n, size)) for q in range(size)]
    snd = torch.from_numpy(mats[rank]).cuda()
    published = 1 if min_run else 0

    def counters():
        return eng.get("MOVE_SEND_DIRECT"), eng.get("MOVE_FUSED")

    # the column type on the send side, 301 doubles per peer on the receive side: block q = rank q's column `rank`
    got = torch.full((size * n,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d0, f0 = counters()
    assert L.mini_alltoall(comm, snd.data_ptr(), 1, col, got.data_ptr(), n, dbl) == 0
    assert counters() == (d0 + published, f0), "the send layout was published, nothing unpacked"
    want = np.stack([mats[q][:, rank] for q in range(size)])          # (size, n): the transposed blocks
    assert got.cpu().numpy().tobytes() == want.tobytes(), "alltoall out of resized columns of doubles"
    # the column type on both sides: column q of my result = rank q's column `rank`
    got2 = torch.full((n, size), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.mini_alltoall(comm, snd.data_ptr(), 1, col, got2.data_ptr(), 1, col) == 0
    assert counters() == (d0 + 2 * published, f0 + 1), "published, and pulled straight into the receive layout"
    assert got2.cpu().numpy().tobytes() == np.ascontiguousarray(want.T).tobytes(), "the block transpose"
    assert snd.cpu().numpy().tobytes() == mats[rank].tobytes(), "the send buffer changed"
    # dense to dense moves neither counter
    flat = torch.from_numpy(np.ascontiguousarray(mats[rank].T)).cuda()
    got3 = torch.zeros(size * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    before = counters()
    assert L.mini_alltoall(comm, flat.data_ptr(), n, dbl, got3.data_ptr(), n, dbl) == 0
    assert counters() == before
    assert got3.cpu().numpy().tobytes() == want.tobytes()
    L.mini_datatype_destroy(col)
    L.mini_comm_destroy(comm)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
