"""One rank of tests/test_move_ddt_ipc_gpu.py: the movement collectives pulling straight into a
derived receive datatype, between processes.

  move_ddt_worker.py engine <key> <rank> <size> <device>   mi355x_alltoallv_ddt / mi355x_gatherv_ddt
  move_ddt_worker.py component <rank> <size> <key>         MPI_Alltoall through coll/mi355x (mini harness)

engine: ranks 0 and 2 receive into a layout (vector(9, 64, 128) of floats; columns of doubles resized
to one element, so the pieces interleave), rank 1 calls the PLAIN form with a dense buffer in the
same collective.  Every rank builds every rank's bytes from the same seeds and compares its own
result byte for byte with the numpy placement of tests/move_ddt_model.py.
"""
from __future__ import annotations

import ctypes
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))
import move_ddt_model as mdl  # noqa: E402

G, POISON = mdl.GUARD, mdl.POISON


def engine_main():
    from conftest import load_pkg
    key, rank, size, dev = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    import torch
    torch.cuda.set_device(dev)
    pkg = load_pkg()
    comm = pkg.Comm.create(key, rank, size, dev)
    plain = rank == 1
    fused = 0

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def sides(name, cnt):
        """layout, byte displacement of every piece, bytes the receive buffer spans"""
        if name == "col8":
            rows, ncols = 33, sum(cnt) + 1
            first = np.concatenate([[0], np.cumsum(cnt[:-1])])
            return mdl.column(rows, ncols), [int(c) * 8 for c in first], rows * ncols * 8
        lay, displs, at = mdl.vec9(), [], 0
        for c in cnt:
            displs.append(at)
            at += lay.span(c) + 48
        return lay, displs, at

    for name in ("vec9", "col8"):
        # ---- alltoallv: receiver r holds counts(r)[q] instances for sender q, all of them sent
        counts = [[1 + (2 * q + r) % 4 for q in range(size)] for r in range(size)]
        lay, displs, total = sides(name, counts[rank])
        sent = [[counts[r][q] * lay.size for r in range(size)] for q in range(size)]   # sent[q][r]
        sdis = [int(v) for v in np.concatenate([[0], np.cumsum(sent[rank][:-1])])]
        data = [[mdl.payload(7000 + 10 * q + r, sent[q][r]) for r in range(size)] for q in range(size)]
        sbuf = dev_of(np.concatenate(data[rank]))
        caps = [sent[q][rank] for q in range(size)]
        doff = [int(v) for v in np.concatenate([[0], np.cumsum(caps[:-1])])]
        rbuf = torch.full(((sum(caps) if plain else total) + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
        want = np.full(rbuf.numel(), POISON, dtype=np.uint8)
        torch.cuda.synchronize()
        if plain:
            comm.alltoallv(sbuf.data_ptr(), sent[rank], sdis, rbuf.data_ptr() + G, caps, doff)
            for q in range(size):
                want[G + doff[q]:G + doff[q] + caps[q]] = data[q][rank]
        else:
            ddt = lay.ddt(pkg)
            comm.alltoallv_ddt(sbuf.data_ptr(), sent[rank], sdis, rbuf.data_ptr() + G, ddt, counts[rank], displs)
            fused += 1
            for q in range(size):
                mdl.place(want, G, lay, displs[q], data[q][rank])
        assert np.array_equal(rbuf.cpu().numpy(), want), f"alltoallv into {name}"
        comm.barrier()
        # ---- gatherv to every root in turn: a layout at roots 0 and 2, dense bytes at root 1
        for root in range(size):
            cnt = counts[root]
            gl, gd, gt = sides(name, cnt)
            gsent = [c * gl.size for c in cnt]
            gdata = [mdl.payload(8000 + 10 * root + q, gsent[q]) for q in range(size)]
            gs = dev_of(gdata[rank])
            goff = [int(v) for v in np.concatenate([[0], np.cumsum(gsent[:-1])])]
            gr = torch.full(((sum(gsent) if plain else gt) + 2 * G,), POISON, dtype=torch.uint8, device="cuda")
            gw = np.full(gr.numel(), POISON, dtype=np.uint8)
            torch.cuda.synchronize()
            am_root = rank == root
            if plain:
                comm.gatherv(gs.data_ptr(), gsent[rank], gr.data_ptr() + G if am_root else None, gsent if am_root else None,
                             goff if am_root else None, root)
                if am_root:
                    for q in range(size):
                        gw[G + goff[q]:G + goff[q] + gsent[q]] = gdata[q]
            else:
                comm.gatherv_ddt(gs.data_ptr(), gsent[rank], gr.data_ptr() + G if am_root else None, gl.ddt(pkg),
                                 cnt if am_root else None, gd if am_root else None, root)
                if am_root:
                    fused += 1
                    for q in range(size):
                        mdl.place(gw, G, gl, gd[q], gdata[q])
            assert np.array_equal(gr.cpu().numpy(), gw), f"gatherv into {name} at root {root}"
            comm.barrier()
    assert comm.get("MOVE_FUSED") == fused, (comm.get("MOVE_FUSED"), fused)
    assert (fused == 0) == plain
    comm.barrier()
    comm.destroy()
    print(f"rank {rank} engine OK", flush=True)


def component_main():
    """MPI_Alltoall, the receive side alone a column type (vector(n, 1, size, MPI_DOUBLE) resized to one
    element): the component hands the layout to the engine, which pulls straight into it"""
    from ddtcases import opal_strided_elems
    from mini import mini
    rank, size, key = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    m = mini()
    L, pkg = m.lib, m.pkg
    vp = ctypes.c_void_p
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    comm = L.mini_comm_create(rank, size, 93)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_stub_module())
    assert L.mini_coll_select(comm, comp) == 90
    m.coll.mca_coll_mi355x_engine_of.restype = vp
    m.coll.mca_coll_mi355x_engine_of.argtypes = [vp]
    eng = pkg.Comm(m.coll.mca_coll_mi355x_engine_of(comm))
    n = 301
    ddt_t = m.dtype_for_slot(pkg.T["DOUBLE"])
    OPAL_FLOAT8 = 16   # opal_datatype_internal.h:107-131 (OPAL_DATATYPE_FLOAT8)
    desc, used, tsize, _, true_ub = opal_strided_elems(n, OPAL_FLOAT8, 8, 8 * size)
    col = L.mini_datatype_create_raw(desc, used, tsize, 0, 8, 0, true_ub, 0)   # MPI_Type_create_resized(.., 0, 8)
    vals = [[np.random.default_rng(9000 + 10 * q + r).standard_normal(n) for r in range(size)] for q in range(size)]
    snd = torch.from_numpy(np.concatenate(vals[rank])).cuda()
    got = torch.full((n * size,), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    before = eng.get("MOVE_FUSED")
    assert L.mini_alltoall(comm, snd.data_ptr(), n, ddt_t, got.data_ptr(), 1, col) == 0
    assert eng.get("MOVE_FUSED") == before + 1, "the component's pull went through the receive layout"
    want = np.stack([vals[q][rank] for q in range(size)], axis=1)     # column q = what rank q sent me
    assert got.cpu().numpy().reshape(n, size).tobytes() == want.tobytes(), "alltoall into resized columns of doubles"
    # a dense receive side stays the plain call
    dense = torch.zeros(n * size, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.mini_alltoall(comm, snd.data_ptr(), n, ddt_t, dense.data_ptr(), n, ddt_t) == 0
    assert eng.get("MOVE_FUSED") == before + 1
    assert dense.cpu().numpy().tobytes() == np.concatenate([vals[q][rank] for q in range(size)]).tobytes()
    L.mini_datatype_destroy(col)
    L.mini_comm_destroy(comm)
    print(f"rank {rank} component OK", flush=True)


if __name__ == "__main__":
    {"engine": engine_main, "component": component_main}[sys.argv[1]]()
