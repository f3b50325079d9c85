"""One rank of tests/test_move_planes_ipc_gpu.py: the movement collectives pulling through row layouts of
two levels (3-D subarrays), between processes.

  move_planes_worker.py engine <key> <rank> <size> <device>   mi355x_alltoallv_ddt2 / mi355x_gatherv_ddt2
  move_planes_worker.py component <rank> <size> <key>         MPI_Alltoall through coll/mi355x (mini harness)

engine: ranks 0 and 2 send through a two-level layout (sub16: 3 rows of 48 B in each of 5 groups; then sub8:
pencils of doubles resized to one element, so the pieces interleave in the sender's memory) and publish it,
rank 1 calls the PLAIN form with dense bytes in the same collective; every receiver takes the two-level
sub4.  Every rank builds every rank's bytes from the same seeds and compares its own result byte for byte
with the numpy model of tests/move_ddt_model.py.
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


def _runs(name, disps, run, nblk, stride, extent):
    return mdl.Layout(name, [(d, run) for d in disps], nblk, stride, extent,
                      lambda pkg: pkg.Ddt.runs(list(disps), [run] * len(disps), nblk, stride, extent))


def sub4():    # the receivers': 3 rows of 12 B at 20 B, 7 groups at 68 B
    return _runs("sub4", [0, 20, 40], 12, 7, 68, 476)


def send_side(name, cnt):
    """layout, byte displacement of every piece, bytes the send buffer spans"""
    if name == "sub8":      # pencils of doubles in a 16 x C array, resized to one element
        C = sum(cnt) + 1
        first = np.concatenate([[0], np.cumsum(cnt[:-1])])
        return _runs("sub8", [0, 8 * C, 16 * C], 8, 4, 32 * C, 8), [int(c) * 8 for c in first], 128 * C
    lay, displs, at = _runs("sub16", [0, 80, 160], 48, 5, 400, 2000), [], 0
    for c in cnt:
        displs.append(at)
        at += lay.span(c) + 48
    return lay, displs, at


def recv_side(nbytes):
    """sub4 instances that cover every piece, their byte displacements, the bytes they span"""
    lay = sub4()
    cnt = [-(-b // lay.size) for b in nbytes]
    displs, at = [], 0
    for c in cnt:
        displs.append(at)
        at += (lay.span(c) + 15) // 16 * 16 + 32
    return lay, cnt, displs, at


def engine_main():
    from conftest import load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg = load_pkg()
    comm = pkg.Comm.create(key, rank, size, dev)
    assert comm.get("MOVE_ROW_LEVELS") == 2, "MI355X_MOVE_ROW_LEVELS sets the knob at creation"
    assert comm.get("MOVE_SEND_MIN_RUN") == 8
    plain = rank == 1
    direct = 0

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def offs(nbytes):
        return [int(v) for v in np.concatenate([[0], np.cumsum(nbytes[:-1])])]

    for name in ("sub16", "sub8"):
        # ---- alltoallv: sender q sends counts[q][r] instances of its layout to r; every receiver takes sub4
        counts = [[1 + (2 * q + r) % 4 for r in range(size)] for q in range(size)]
        lay, sdis, total = send_side(name, counts[rank])
        assert lay.ddt(pkg).row_levels() == 2
        size1 = lay.size
        data = [[mdl.payload(7000 + 10 * q + r, counts[q][r] * size1) for r in range(size)] for q in range(size)]
        sent = [counts[rank][r] * size1 for r in range(size)]
        rl, rcnt, rdis, rtotal = recv_side([counts[q][rank] * size1 for q in range(size)])
        rbuf = torch.full((rtotal + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
        want = np.full(rbuf.numel(), POISON, dtype=np.uint8)
        for q in range(size):
            mdl.place(want, G, rl, rdis[q], data[q][rank])
        rddt = rl.ddt(pkg)
        if plain:
            host = np.concatenate(data[rank])
            sbuf = dev_of(host)
            torch.cuda.synchronize()
            comm.alltoallv_ddt(sbuf.data_ptr(), sent, offs(sent), rbuf.data_ptr() + G, rddt, rcnt, rdis)
        else:
            host = np.full(total + 2 * G, FILL, dtype=np.uint8)
            for r in range(size):
                host[G + sdis[r] + lay.offsets(sent[r])] = data[rank][r]
            sbuf = dev_of(host)
            torch.cuda.synchronize()
            comm.alltoallv_ddt2(sbuf.data_ptr() + G, lay.ddt(pkg), counts[rank], sdis, rbuf.data_ptr() + G, rddt, rcnt, rdis)
            direct += 1
        assert np.array_equal(rbuf.cpu().numpy(), want), f"alltoallv out of {name}"
        assert np.array_equal(sbuf.cpu().numpy(), host), f"alltoallv out of {name}: the send buffer changed"
        comm.barrier()
        # ---- gatherv to every root in turn: the root takes sub4
        for root in range(size):
            cnt = counts[root]
            gl, gd, gt = send_side(name, [cnt[rank]])
            gdata = [mdl.payload(8000 + 10 * root + q, cnt[q] * gl.size) for q in range(size)]
            gcap = [len(d) for d in gdata]
            am_root = rank == root
            rl, rcnt, rdis, rtotal = recv_side(gcap)
            gr = torch.full((rtotal + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
            gw = np.full(gr.numel(), POISON, dtype=np.uint8)
            if am_root:
                for q in range(size):
                    mdl.place(gw, G, rl, rdis[q], gdata[q])
            rargs = (gr.data_ptr() + G, rl.ddt(pkg), rcnt, rdis) if am_root else (None, None, None, None)
            if plain:
                gs = dev_of(gdata[rank])
                torch.cuda.synchronize()
                comm.gatherv_ddt(gs.data_ptr(), gcap[rank], rargs[0], rargs[1], rargs[2], rargs[3], root)
            else:
                gh = np.full(gt + 2 * G, FILL, dtype=np.uint8)
                gh[G + gl.offsets(gcap[rank])] = gdata[rank]
                gs = dev_of(gh)
                torch.cuda.synchronize()
                comm.gatherv_ddt2(gs.data_ptr() + G, gl.ddt(pkg), cnt[rank], rargs[0], rargs[1], rargs[2], rargs[3], root)
                direct += 1
            assert np.array_equal(gr.cpu().numpy(), gw), f"gatherv out of {name} at root {root}"
            comm.barrier()
    assert comm.get("MOVE_SEND_DIRECT") == direct, (comm.get("MOVE_SEND_DIRECT"), direct)
    assert (direct == 0) == plain
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    """MPI_Alltoall of the z-pencils of an nz x ny x nx array of floats: the send type is the 3-D subarray
    hvector(sz, 1, plane, vector(sy, sx, nx, FLOAT4)) resized to one pencil's width, so the pieces interleave in
    the sender's memory.  The component hands the layout to the engine, which publishes it under
    coll_mi355x_move_row_levels = 2 (with 1 the component packs: the same bytes, MOVE_SEND_DIRECT stays); then
    the subarray on both sides -- nothing packed, nothing unpacked"""
    from ddtcases import OPAL_FLOAT4, rec_elem, rec_end, rec_loop
    from mini import mini
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    levels = int(os.environ["OMPI_MCA_coll_mi355x_move_row_levels"])
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
    assert eng.get("MOVE_ROW_LEVELS") == levels, "coll_mi355x_move_row_levels reaches the engine"
    assert eng.get("MOVE_SEND_MIN_RUN") == 8
    # the array and the pencil: sz x sy x sx floats out of nz x ny x nx, one spare column and one spare row
    sz, sy, sx = 5, 3, 3
    nz, ny, nx = sz, sy + 1, size * sx + 1
    row, plane = nx * 4, ny * nx * 4
    flt = m.dtype_for_slot(pkg.T["FLOAT"])
    # hvector(sz, 1, plane, vector(sy, sx, nx, FLOAT4)) as opal describes it: LOOP sz { LOOP sy { ELEM sx } }
    desc = (rec_loop(sz, 4, plane) + rec_loop(sy, 2, row) + rec_elem(OPAL_FLOAT4, sx, 4, 0) + rec_end(2, sx * 4, 0) +
            rec_end(4, sy * sx * 4, 0))
    true_ub = (sz - 1) * plane + (sy - 1) * row + sx * 4
    pencil = L.mini_datatype_create_raw(desc, 5, sz * sy * sx * 4, 0, sx * 4, 0, true_ub, 0)   # resized to (0, sx floats)
    arrs = [np.random.default_rng(9300 + q).standard_normal((nz, ny, nx)).astype(np.float32) for q in range(size)]
    snd = torch.from_numpy(arrs[rank]).cuda()
    published = 1 if levels == 2 else 0
    per = sz * sy * sx

    def counters():
        return eng.get("MOVE_SEND_DIRECT"), eng.get("MOVE_FUSED")

    def block(q, r):     # what rank q sends to rank r: its pencil r
        return arrs[q][:sz, :sy, r * sx:(r + 1) * sx]

    # the subarray on the send side, dense floats on the receive side: block q = rank q's pencil `rank`
    got = torch.full((size * per,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    d0, f0 = counters()
    assert L.mini_alltoall(comm, snd.data_ptr(), 1, pencil, got.data_ptr(), per, flt) == 0
    assert counters() == (d0 + published, f0), "the send layout was published (or packed), nothing unpacked"
    want = np.stack([block(q, rank) for q in range(size)])
    assert got.cpu().numpy().tobytes() == want.tobytes(), "alltoall out of z-pencils of floats"
    # the subarray on both sides: pencil q of my result = rank q's pencil `rank`
    got2 = torch.full((nz, ny, nx), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert L.mini_alltoall(comm, snd.data_ptr(), 1, pencil, got2.data_ptr(), 1, pencil) == 0
    assert counters() == (d0 + 2 * published, f0 + 1), "published, and pulled straight into the receive layout"
    want2 = np.full((nz, ny, nx), -1.0, dtype=np.float32)
    for q in range(size):
        want2[:sz, :sy, q * sx:(q + 1) * sx] = block(q, rank)
    assert got2.cpu().numpy().tobytes() == want2.tobytes(), "the transpose of pencils"
    assert snd.cpu().numpy().tobytes() == arrs[rank].tobytes(), "the send buffer changed"
    L.mini_datatype_destroy(pencil)
    L.mini_comm_destroy(comm)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
