"""One rank of tests/test_movement_paths_gpu.py: which path each data-movement entry point of
coll/mi355x takes, through the mini harness with the host module installed below the component.

  movement_paths_worker.py <rank> <size> <key> <mixed>

One loop over {allgather, bcast, gather, gatherv, scatter, scatterv, allgatherv, alltoall, alltoallv} x
{not in place, in place (where MPI has it; a rooted call: on the root only)}, plus iallgather and
ibcast, root = 2, MPI_INT, 5 elements per piece, vector counts [5, 0, 3] (rank 1 sends and receives
nothing) at displacements with a gap of 2 between pieces, every buffer padded with 4 sentinel
elements, runs under these scenarios:
  (a) every rank on device buffers: the engine serves the call;
  (b) rank 0 on host buffers among device ranks, after device use (<mixed> = 1 only): the engine
      serves the call, the host rank joins it on device copies;
  (c) after a window of 32 host-only calls the buffer-kind vote says host (<mixed> = 1 only, the
      blocking calls): rank 0 on host buffers, ranks 1 and 2 on device -- the previous owner serves
      the call, each device rank stages its buffers through host memory exactly once.  bcast,
      allgather, gather and alltoall really run in the host module: exact data.  scatter and the four
      vector forms land on the stub: the call returns its marker and nothing is copied back;
  (d) <mixed> = 0: iallgather with a host sbuf and a device rbuf, ibcast on host buffers: the host
      module's nonblocking slots serve them, the device rbuf staged;
  (e) bad arguments go to the previous owner without a vote;
  (f) a displacement of -1 on a device rank of (c): OMPI_ERR_NOT_SUPPORTED, nothing staged.
mca_coll_mi355x_staged_calls, mini_host_calls and mini_stub_calls say which path ran; results are exact
against numpy placement, gaps and padding keep the sentinel, send buffers keep their contents.
"""
from __future__ import annotations

import ctypes
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).parent))

K, VCOUNTS, ROOT, GAP = 5, [5, 0, 3], 2, 2
SENTINEL, PAD, WINDOW = -9, 4, 32
IN_PLACE = 1
OMPI_ERR_BAD_PARAM, OMPI_ERR_NOT_SUPPORTED = -5, -8
BLOCKING = ("allgather", "bcast", "gather", "gatherv", "scatter", "scatterv", "allgatherv", "alltoall", "alltoallv")
NONBLOCKING = ("iallgather", "ibcast")
ROOTED = ("bcast", "gather", "gatherv", "scatter", "scatterv")
HOST_ID = {"bcast": 4, "allgather": 3, "iallgather": 13, "ibcast": 14}   # mini_host_calls
STUB_ID = {"gatherv": 10, "scatterv": 11, "allgatherv": 12, "alltoallv": 13, "scatter": 7}   # mini_stub_calls


def val(r, q, k):
    """the k elements rank r sends to rank q"""
    return (1 + np.arange(k) + 100 * q + 10000 * r).astype(np.int32)


def disps(counts):
    return [sum(counts[:q]) + GAP * q for q in range(len(counts))]


def place(pieces, at=None):
    """the pieces at their displacements (None: consecutive), sentinel in the gaps and in the padding"""
    at = at if at is not None else [sum(len(p) for p in pieces[:q]) for q in range(len(pieces))]
    out = np.full(max(a + len(p) for a, p in zip(at, pieces)) + PAD, SENTINEL, np.int32)
    for a, p in zip(at, pieces):
        out[a:a + len(p)] = p
    return out


def only(q, pieces, at=None):
    """place() with every piece but q left as sentinel (an in-place receive buffer before the call)"""
    return place([p if i == q else np.full(len(p), SENTINEL, np.int32) for i, p in enumerate(pieces)], at)


class Plan:
    """one call on one rank: send / recv are the buffers' contents before it (None: no buffer, NULL or
    MPI_IN_PLACE as `inplace` says), want the receive buffer after it (None: as it was), run(L, comm,
    sp, rp, req) makes it"""

    def __init__(self, c, inplace, me, n):
        IA = lambda v: (ctypes.c_int * n)(*v)
        base = c[1:] if c in NONBLOCKING else c
        root = me == ROOT
        self.send_inplace = self.recv_inplace = False
        vd = disps(VCOUNTS)
        a2a = [min(VCOUNTS[me], VCOUNTS[q]) for q in range(n)]   # symmetric: what me sends q, q sends me
        ad = disps(a2a)
        if base == "bcast":
            self.send, self.receives = None, True
            self.recv = place([val(ROOT, 0, K)]) if root else place([np.full(K, SENTINEL, np.int32)])
            self.want = place([val(ROOT, 0, K)])
            self.run = lambda L, comm, dt, sp, rp, req: L.mini_ibcast(comm, rp, K, dt, ROOT, req) if req else \
                L.mini_bcast(comm, rp, K, dt, ROOT)
            return
        # (send pieces, their displacements), (received pieces, their displacements), the piece of the
        # receive buffer an in-place call reads (None: all of them), who receives
        if base in ("allgather", "gather"):
            snd, rcv, mine = ([val(me, 0, K)], None), ([val(q, 0, K) for q in range(n)], None), me
        elif base in ("allgatherv", "gatherv"):
            snd, rcv, mine = ([val(me, 0, VCOUNTS[me])], None), ([val(q, 0, VCOUNTS[q]) for q in range(n)], vd), me
        elif base == "scatter":
            snd, rcv = ([val(ROOT, q, K) for q in range(n)], None), ([val(ROOT, me, K)], None)
        elif base == "scatterv":
            snd, rcv = ([val(ROOT, q, VCOUNTS[q]) for q in range(n)], vd), ([val(ROOT, me, VCOUNTS[me])], None)
        elif base == "alltoall":
            snd, rcv, mine = ([val(me, q, K) for q in range(n)], None), ([val(q, me, K) for q in range(n)], None), None
        else:
            snd, rcv, mine = ([val(me, q, a2a[q]) for q in range(n)], ad), ([val(q, me, a2a[q]) for q in range(n)], ad), None
        receives = root if base in ("gather", "gatherv") else True
        sends = root if base in ("scatter", "scatterv") else True
        self.receives = receives
        self.send = place(*snd) if sends else None
        self.recv = place([np.full(len(p), SENTINEL, np.int32) for p in rcv[0]], rcv[1])
        self.want = place(*rcv) if receives else None
        if inplace and base in ("scatter", "scatterv"):   # the root keeps its own piece where it is
            self.recv, self.want, self.recv_inplace = None, None, True
        elif inplace:                                     # the receive buffer holds this rank's input
            self.send, self.send_inplace = None, True
            self.recv = place(*snd) if mine is None else only(mine, *rcv)
        r = ROOT
        self.run = {
            "allgather": lambda L, comm, dt, sp, rp, req: L.mini_iallgather(comm, sp, K, dt, rp, K, dt, req) if req else
            L.mini_allgather(comm, sp, K, dt, rp, K, dt),
            "gather": lambda L, comm, dt, sp, rp, req: L.mini_gather(comm, sp, K, dt, rp, K, dt, r),
            "gatherv": lambda L, comm, dt, sp, rp, req: L.mini_gatherv(comm, sp, VCOUNTS[me], dt, rp, IA(VCOUNTS), IA(vd), dt, r),
            "scatter": lambda L, comm, dt, sp, rp, req: L.mini_scatter(comm, sp, K, dt, rp, K, dt, r),
            "scatterv": lambda L, comm, dt, sp, rp, req: L.mini_scatterv(comm, sp, IA(VCOUNTS), IA(vd), dt, rp, VCOUNTS[me], dt, r),
            "allgatherv": lambda L, comm, dt, sp, rp, req: L.mini_allgatherv(comm, sp, VCOUNTS[me], dt, rp, IA(VCOUNTS), IA(vd), dt),
            "alltoall": lambda L, comm, dt, sp, rp, req: L.mini_alltoall(comm, sp, K, dt, rp, K, dt),
            "alltoallv": lambda L, comm, dt, sp, rp, req: L.mini_alltoallv(comm, sp, IA(a2a), IA(ad), dt, rp, IA(a2a), IA(ad), dt),
        }[base]


def main():
    from mini import mini
    rank, size, key, mixed = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
    assert size == len(VCOUNTS)
    import torch
    torch.cuda.set_device(rank % torch.cuda.device_count())
    m = mini()
    L, pkg = m.lib, m.pkg
    vp = ctypes.c_void_p
    L.mini_host_module.restype = vp
    L.mini_host_calls.argtypes = [ctypes.c_int]
    comp = m.component_ptr(m.coll, "mca_coll_mi355x_component")
    assert L.mini_component_register(comp) == 0
    assert ctypes.c_int.in_dll(m.coll, "mca_coll_mi355x_mixed_buffers").value == mixed
    comm = L.mini_comm_create(rank, size, 95)
    assert L.mini_comm_set_channel(comm, key.encode()) == 0
    L.mini_comm_install(comm, L.mini_host_module())
    assert L.mini_coll_select(comm, comp) == 90
    staged = ctypes.c_ulong.in_dll(m.coll, "mca_coll_mi355x_staged_calls")
    idt = m.dtype_for_slot(pkg.T["INT32"])
    marker = L.mini_stub_marker()
    votes = [0]   # buffer-kind votes taken on comm: one per blocking call whose arguments are good
    q = vp()

    def put(a, on_host):
        if on_host:
            h = np.ascontiguousarray(a).copy()
            return h, h.ctypes.data, (lambda: h.copy())
        d = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
        return d, d.data_ptr(), (lambda: d.cpu().numpy().view(a.dtype).copy())

    def counters(c):
        return (staged.value, L.mini_host_calls(HOST_ID[c]) if c in HOST_ID else 0,
                L.mini_stub_calls(STUB_ID[c]) if c in STUB_ID else 0)

    def variants(c):
        return (False,) if c.endswith("bcast") else (False, True)

    def run(name, c, inplace, on_host, by_host):
        """by_host: the previous owner serves the call (else the engine: no counter moves)"""
        what = f"({name}) {c} inplace={inplace}"
        p = Plan(c, inplace and (c not in ROOTED or rank == ROOT), rank, size)
        keep_s, sp, read_s = (None, IN_PLACE if p.send_inplace else None, None) if p.send is None else put(p.send, on_host)
        # (a non-root's rbuf is not significant; the stub looks at every pointer it is handed, so on the
        # way to it there is none)
        keep_r, rp, read_r = (None, IN_PLACE if p.recv_inplace else None, None) \
            if p.recv is None or (by_host and not p.receives) else put(p.recv, on_host)
        torch.cuda.synchronize()
        before = counters(c)
        nb = c in NONBLOCKING
        rc = p.run(L, comm, idt, sp, rp, ctypes.byref(q) if nb else None)
        votes[0] += not nb
        stub = by_host and c in STUB_ID
        assert rc == (marker if stub else 0), (what, rc)
        if nb:
            assert L.mini_wait(ctypes.byref(q)) == 0, what
        moved = tuple(b - a for a, b in zip(before, counters(c)))
        dev_bufs = not on_host and (sp not in (None, IN_PLACE) or rp not in (None, IN_PLACE))
        assert moved == ((int(dev_bufs), int(c in HOST_ID), int(c in STUB_ID)) if by_host else (0, 0, 0)), (what, moved)
        if read_s:
            assert np.array_equal(read_s(), p.send), what + ": the send buffer changed"
        if read_r:   # a call that did not succeed copies nothing back; a non-root's rbuf is not significant
            want = p.recv if stub or p.want is None else p.want
            assert np.array_equal(read_r(), want), (what, read_r(), want)

    def host_window():
        """to the next checkpoint of the vote, then a whole window of host-only calls: the window after
        it is one in which the device ranks wait and a mixed call runs on the host"""
        fill = (-votes[0]) % WINDOW + WINDOW
        for _ in range(fill):
            h = np.full(1, 7 if rank == 0 else -1, np.int32)
            assert L.mini_bcast(comm, h.ctypes.data, 1, idt, 0) == 0 and h[0] == 7
        votes[0] += fill

    for c in BLOCKING + NONBLOCKING:
        for ip in variants(c):
            run("a", c, ip, False, False)
    if mixed:
        run("b: device use first", "allgather", False, False, False)
        for c in BLOCKING + NONBLOCKING:
            for ip in variants(c):
                run("b", c, ip, rank == 0, False)
        # (c): every call between two checkpoints of the vote, the bad displacement (f) as the last one
        todo = [(c, ip) for c in BLOCKING for ip in variants(c)]
        room = WINDOW - 1
        for i in range(0, len(todo), room - 1):
            host_window()
            for c, ip in todo[i:i + room - 1]:
                run("c", c, ip, rank == 0, True)
        assert votes[0] % WINDOW < room, "no room left in this window for (f)"
        p = Plan("allgatherv", False, rank, size)
        keep_s, sp, _ = put(p.send, rank == 0)
        keep_r, rp, read_r = put(p.recv, rank == 0)
        torch.cuda.synchronize()
        before = counters("allgatherv")
        IA = ctypes.c_int * size
        rc = L.mini_allgatherv(comm, sp, VCOUNTS[rank], idt, rp, IA(*VCOUNTS), IA(0, -1, K + GAP), idt)
        votes[0] += 1
        moved = tuple(b - a for a, b in zip(before, counters("allgatherv")))
        if rank == 0:   # host buffers: the stub's to answer
            assert (rc, moved) == (marker, (0, 0, 1)), ("(f)", rc, moved)
        else:
            assert (rc, moved) == (OMPI_ERR_NOT_SUPPORTED, (0, 0, 0)), ("(f)", rc, moved)
        assert np.array_equal(read_r(), p.recv), "(f): rbuf changed"
    else:
        # (d): one buffer kind per call -- a host side sends the call to the host module's nonblocking slot
        p = Plan("iallgather", False, rank, size)
        keep_r, rp, read_r = put(p.recv, False)
        torch.cuda.synchronize()
        before = counters("iallgather")
        assert L.mini_iallgather(comm, p.send.ctypes.data, K, idt, rp, K, idt, ctypes.byref(q)) == 0
        assert L.mini_wait(ctypes.byref(q)) == 0
        moved = tuple(b - a for a, b in zip(before, counters("iallgather")))
        assert moved == (1, 1, 0) and np.array_equal(read_r(), p.want), ("(d) iallgather", moved, read_r())
        run("d", "ibcast", False, True, True)
    # (e): bad arguments are the previous owner's to answer, on this rank alone -- no vote
    h = np.full(K + PAD, SENTINEL, np.int32)
    for c, call in (("bcast", lambda: L.mini_bcast(comm, h.ctypes.data, -1, idt, ROOT)),
                    ("allgather", lambda: L.mini_allgather(comm, h.ctypes.data, K, idt, h.ctypes.data, -1, idt))):
        before = counters(c)
        rc = call()
        moved = tuple(b - a for a, b in zip(before, counters(c)))
        assert (rc, moved) == (OMPI_ERR_BAD_PARAM, (0, 1, 0)), ("(e)", c, rc, moved)
    # MPI_IN_PLACE on a non-root of gather, over the stub (its gather keeps a counter).  The root makes no
    # call: its arguments would be good ones, and it would vote alone and wait for the others for ever.
    bad = L.mini_comm_create(rank, size, 96)
    assert L.mini_comm_set_channel(bad, (key + "_bad").encode()) == 0
    L.mini_comm_install(bad, L.mini_stub_module())
    assert L.mini_coll_select(bad, comp) == 90
    if rank != ROOT:
        before = (staged.value, L.mini_stub_calls(7))
        rc = L.mini_gather(bad, IN_PLACE, K, idt, h.ctypes.data, K, idt, ROOT)
        assert (rc, staged.value - before[0], L.mini_stub_calls(7) - before[1]) == (marker, 0, 1), ("(e) gather", rc)
    assert (h == SENTINEL).all()
    assert L.mini_device_hits() == 0, "a device pointer reached the host module"
    L.mini_comm_destroy(bad)
    L.mini_comm_destroy(comm)
    print(f"rank {rank} paths OK", flush=True)


if __name__ == "__main__":
    main()
