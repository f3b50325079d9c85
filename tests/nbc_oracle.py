"""Test-side reference for coll/libnbc's nonblocking reductions: a small message-passing simulator.

Every rank gets the schedule libnbc would build for it -- rounds of send / recv / op / copy
separated by barriers -- restated from nbc_iallreduce.c (allred_sched_diss :225-302,
allred_sched_ring :304-471), nbc_ireduce.c (red_sched_binomial :223-285, red_sched_chain :288-340)
and coll_libnbc_ireduce_scatter_block.c (:62-138).  The schedules then run over numpy buffers the
way NBC_Start_round / NBC_Progress run them (nbc.c:380-520): the actions of a round start in order
(an op or a copy runs at once, a send takes the buffer as it is), the round ends when its receives
have arrived, messages between two ranks arrive in posting order.  Each op is
NBC_Sched_op(target, in1, in2) = ompi_3buff_op_reduce(op, in1, in2, target) (nbc.c:123-145,
:446-467), run here by the oracle's 3-buff loop into a scratch array and copied back, because
libnbc lets the target alias an operand.

Nothing here is shared with the engine's expression builders (csrc/rt/coll_nbc.cpp): the engine
derives one expression per element, this file moves data.
"""
from __future__ import annotations

import math
from collections import defaultdict, deque

import numpy as np

BINOMIAL, RING, CHAIN = 101, 102, 103
_LOG2 = 0.69314718055994530941   # nbc_internal.h:45


def iallreduce_alg(p: int, count: int, esz: int, inplace: bool) -> int:
    """nbc_iallreduce.c:80-85"""
    return BINOMIAL if (p < 4 or esz * count < 65536 or inplace) else RING


def ireduce_alg(p: int, count: int, esz: int) -> int:
    """nbc_ireduce.c:74-88"""
    return BINOMIAL if (p > 4 or esz * count < 65536) else CHAIN


def ring_segments(count: int, p: int) -> list[tuple[int, int]]:
    """(offset, size) of the p segments, nbc_iallreduce.c:311-329"""
    segsize = count // p
    if count % p != 0:
        segsize += 1
    mycount = count
    sizes, offs = [], [0]
    for i in range(p):
        mycount -= segsize
        sizes.append(segsize)
        if mycount < 0:
            sizes[i] = segsize + mycount
            mycount = 0
        if i:
            offs.append(offs[i - 1] + sizes[i - 1])
    return list(zip(offs, sizes))


def _vrank(rank, root):      # RANK2VRANK
    v = rank
    if rank == 0:
        v = root
    if rank == root:
        v = 0
    return v


def _rank(vrank, root):      # VRANK2RANK
    r = vrank
    if vrank == 0:
        r = root
    if vrank == root:
        r = 0
    return r


def _maxr(p):
    return int(math.ceil(math.log(p) / _LOG2))


class Sim:
    """p ranks, each with named numpy buffers and a schedule"""

    def __init__(self, oracle, op: int, ty: int, p: int):
        self.oracle, self.op, self.ty, self.p = oracle, op, ty, p
        self.buf = [dict() for _ in range(p)]
        self.rounds = [[[]] for _ in range(p)]

    # ---- schedule construction (NBC_Sched_*)
    def send(self, r, ref, cnt, peer):
        self.rounds[r][-1].append(("send", ref, cnt, peer))

    def recv(self, r, ref, cnt, peer):
        self.rounds[r][-1].append(("recv", ref, cnt, peer))

    def op3(self, r, tgt, in1, in2, cnt):
        self.rounds[r][-1].append(("op", tgt, in1, in2, cnt))

    def copy(self, r, src, dst, cnt):
        self.rounds[r][-1].append(("copy", src, dst, cnt))

    def barrier(self, r):
        self.rounds[r].append([])

    # ---- execution
    def _view(self, r, ref, cnt):
        name, off = ref
        return self.buf[r][name][off:off + cnt]

    def _start(self, r, actions, chan, pending):
        for a in actions:
            if a[0] == "send":
                chan[(r, a[3])].append(self._view(r, a[1], a[2]).copy())
            elif a[0] == "recv":
                pending.append(a)
            elif a[0] == "op":
                _, tgt, in1, in2, cnt = a
                if cnt == 0:
                    continue
                x1 = np.ascontiguousarray(self._view(r, in1, cnt)).copy()
                x2 = np.ascontiguousarray(self._view(r, in2, cnt)).copy()
                out = self._view(r, tgt, cnt).copy()   # (members 3-buff leaves alone keep the target's bytes)
                self.oracle.oracle_op_3buff(self.op, self.ty, x1.ctypes.data, x2.ctypes.data, out.ctypes.data, cnt)
                self._view(r, tgt, cnt)[:] = out
            else:
                _, src, dst, cnt = a
                self._view(r, dst, cnt)[:] = self._view(r, src, cnt).copy()

    def run(self):
        p = self.p
        pos, started = [0] * p, [False] * p
        pending = [[] for _ in range(p)]
        chan = defaultdict(deque)
        while True:
            moved = False
            for r in range(p):
                if pos[r] >= len(self.rounds[r]):
                    continue
                if not started[r]:
                    self._start(r, self.rounds[r][pos[r]], chan, pending[r])
                    started[r] = moved = True
                still, blocked = [], set()
                for a in pending[r]:
                    q = chan[(a[3], r)]
                    if a[3] in blocked or not q:
                        blocked.add(a[3])
                        still.append(a)
                        continue
                    data = q.popleft()
                    assert len(data) == a[2], "message length differs from the receive's"
                    self._view(r, a[1], a[2])[:] = data
                    moved = True
                pending[r] = still
                if not still:
                    pos[r] += 1
                    started[r] = False
                    moved = True
            if all(pos[r] >= len(self.rounds[r]) for r in range(p)):
                return
            assert moved, "the schedule deadlocks"


def _binomial_up(sim, r, p, root, count, red):
    """the reduce rounds shared by the three binomial schedules; `red` names the buffer a rank
    reduces into.  Returns nothing: the result ends in `red` of rank `root`."""
    vrank = _vrank(r, root)
    firstred = True
    for k in range(1, _maxr(p) + 1):
        if vrank % (1 << k) == 0:
            peer = _rank(vrank + (1 << (k - 1)), root)
            if peer < p:
                sim.recv(r, ("tmp", 0), count, peer)
                sim.barrier(r)
                sim.op3(r, (red, 0), ("send", 0) if firstred else (red, 0), ("tmp", 0), count)
                firstred = False
                sim.barrier(r)
        else:
            peer = _rank(vrank - (1 << (k - 1)), root)
            sim.send(r, ("send", 0) if firstred else (red, 0), count, peer)
            break


def iallreduce(oracle, op, ty, xs, esz, inplace=False, alg=None):
    """returns (every rank's recvbuf, the algorithm); alg: run that schedule whatever libnbc selects"""
    p, count = len(xs), len(xs[0])
    alg = alg or iallreduce_alg(p, count, esz, inplace)
    sim = Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        b["recv"] = xs[r].copy() if inplace else np.zeros_like(xs[r])
        b["send"] = b["recv"] if inplace else xs[r].copy()   # NBC_IN_PLACE: sendbuf = recvbuf
        b["tmp"] = np.zeros_like(xs[r])
        if p == 1:
            if not inplace:
                b["recv"][:] = b["send"]
            continue
        if alg == BINOMIAL:
            _binomial_up(sim, r, p, 0, count, "recv")
            vrank, maxr = r, _maxr(p)        # root 0: vrank == rank; the bcast down
            if vrank != 0:
                for k in range(maxr):
                    if (1 << k) <= vrank < (1 << (k + 1)):
                        sim.recv(r, ("recv", 0), count, vrank - (1 << k))
                sim.barrier(r)
            for k in range(maxr):
                if (vrank + (1 << k) < p and vrank < (1 << k)) or vrank == 0:
                    sim.send(r, ("recv", 0), count, vrank + (1 << k))
        else:
            seg = ring_segments(count, p)
            speer, rpeer = (r + 1) % p, (r - 1 + p) % p
            for rnd in range(2 * p - 2):
                se, re = (r + 1 - rnd + 2 * p) % p, (r - rnd + 2 * p) % p
                sim.send(r, ("send" if rnd == 0 else "recv", seg[se][0]), seg[se][1], speer)
                sim.recv(r, ("recv", seg[re][0]), seg[re][1], rpeer)
                sim.barrier(r)
                if rnd < p - 1:
                    sim.op3(r, ("recv", seg[re][0]), ("send", seg[re][0]), ("recv", seg[re][0]), seg[re][1])
                    sim.barrier(r)
    sim.run()
    return [sim.buf[r]["recv"] for r in range(p)], alg


def ireduce(oracle, op, ty, xs, esz, root, inplace=False, alg=None):
    """returns (the root's recvbuf, the algorithm); inplace: MPI_IN_PLACE at the root; alg as above"""
    p, count = len(xs), len(xs[0])
    alg = alg or ireduce_alg(p, count, esz)
    sim = Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        if r == root:
            b["recv"] = xs[r].copy() if inplace else np.zeros_like(xs[r])
        b["send"] = b["recv"] if (inplace and r == root) else xs[r].copy()
        b["tmp"] = np.zeros_like(xs[r])
        b["red"] = np.zeros_like(xs[r])   # the second half of a non-root's tmpbuf
        if p == 1:
            if not inplace:
                b["recv"][:] = b["send"]
            continue
        if alg == BINOMIAL:
            _binomial_up(sim, r, p, root, count, "recv" if r == root else "red")
            continue
        vrank = _vrank(r, root)
        rpeer, speer = _rank(vrank + 1, root), _rank(vrank - 1, root)
        fragsize = 16384 // 2
        numfrag = count * esz // fragsize
        if (count * esz) % fragsize != 0:
            numfrag += 1
        fragcount = count // numfrag
        for f in range(numfrag):
            off = f * fragcount
            this = count - fragcount * f if f == numfrag - 1 else fragcount
            if vrank != p - 1:
                sim.recv(r, ("tmp", off), this, rpeer)
                sim.barrier(r)
                sim.op3(r, ("recv" if vrank == 0 else "tmp", off), ("send", off), ("tmp", off), this)
                sim.barrier(r)
            if vrank != 0:
                sim.send(r, ("send" if vrank == p - 1 else "tmp", off), this, speer)
                sim.barrier(r)
    sim.run()
    return sim.buf[root]["recv"], alg


def ireduce_scatter_block(oracle, op, ty, xs, rcount, inplace=False):
    """returns (every rank's recvbuf[:rcount], BINOMIAL)"""
    p, count = len(xs), len(xs[0])
    assert count == p * rcount and p > 1
    sim = Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        b["recv"] = xs[r].copy() if inplace else np.zeros(rcount, dtype=xs[r].dtype)
        b["send"] = b["recv"] if inplace else xs[r].copy()
        b["tmp"] = np.zeros_like(xs[r])
        b["red"] = np.zeros_like(xs[r])
        _binomial_up(sim, r, p, 0, count, "red")
        sim.barrier(r)
        if r != 0:
            sim.recv(r, ("recv", 0), rcount, 0)
        else:
            for q in range(1, p):
                sim.send(r, ("red", q * rcount), rcount, q)
            sim.copy(r, ("red", 0), ("recv", 0), rcount)
    sim.run()
    return [sim.buf[r]["recv"][:rcount] for r in range(p)], BINOMIAL


def tie_nan_pairs(dtype, n, salt):
    """MAXLOC / MINLOC data on which the 2-buff and 3-buff rules differ: values from {NaN, -0.0,
    +0.0, 1.0, 2.0} (ties between zeros of either sign, unordered compares), random indices"""
    rng = np.random.default_rng(0xB1D0 + salt)
    x = np.zeros(n, dtype=dtype)
    x["v"] = rng.choice(np.array([np.nan, -0.0, 0.0, 1.0, 2.0], dtype=dtype["v"]), n)
    x["k"] = rng.integers(-50, 50, n, dtype=np.int32)
    return x
