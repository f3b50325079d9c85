"""Test-side reference for coll/libnbc's MPI_Iscan and MPI_Iexscan, on the message-passing
simulator of tests/nbc_oracle.py (send / recv / op3 / copy / barrier run the way NBC_Progress runs
them).

The two schedules are restated from nbc_iscan.c:67-105 and nbc_iexscan.c:94-135.  Both are the
rank chain: rank r receives the partial of ranks 0..r-1 from rank r-1, combines it with its own
data as NBC_Sched_op(target, in1 = sendbuf, in2 = the received partial) -- ompi_3buff_op_reduce --
and sends the result on to rank r+1.  Iscan keeps that result (rank 0 a copy of its input);
Iexscan keeps what it received (rank 0's recvbuf is never written, the last rank reduces nothing).
"""
from __future__ import annotations

import numpy as np

from nbc_oracle import Sim


def iscan(oracle, op, ty, xs, inplace=False):
    """every rank's recvbuf after MPI_Iscan"""
    p, count = len(xs), len(xs[0])
    sim = Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        b["recv"] = xs[r].copy() if inplace else np.zeros_like(xs[r])
        b["send"] = b["recv"] if inplace else xs[r].copy()   # NBC_IN_PLACE: sendbuf = recvbuf
        b["tmp"] = np.zeros_like(xs[r])
        if r == 0 and not inplace:
            b["recv"][:] = b["send"]                          # NBC_Copy at initiation (:67-71)
        if r != 0:
            sim.recv(r, ("tmp", 0), count, r - 1)
            sim.barrier(r)
            sim.op3(r, ("recv", 0), ("send", 0), ("tmp", 0), count)
            sim.barrier(r)
        if r != p - 1:
            sim.send(r, ("recv", 0), count, r + 1)
    sim.run()
    return [sim.buf[r]["recv"] for r in range(p)]


def iexscan(oracle, op, ty, xs, before, inplace=False):
    """every rank's recvbuf after MPI_Iexscan; `before`: what the recvbufs held (in place: the inputs)"""
    p, count = len(xs), len(xs[0])
    sim = Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        b["recv"] = xs[r].copy() if inplace else before[r].copy()
        b["send"] = b["recv"] if inplace else xs[r].copy()
        b["tmp"] = np.zeros_like(xs[r])
        b["tmp2"] = np.zeros_like(xs[r])                      # the second half of an in-place tmpbuf
        if r != 0:
            held = "tmp2" if (inplace and r < p - 1) else "recv"
            sim.recv(r, (held, 0), count, r - 1)
            if r < p - 1:
                sim.barrier(r)
                sim.op3(r, ("tmp", 0), ("send", 0), (held, 0), count)
                sim.barrier(r)
                sim.send(r, ("tmp", 0), count, r + 1)
                if inplace:
                    sim.copy(r, ("tmp2", 0), ("recv", 0), count)
        elif p > 1:
            sim.send(r, ("send", 0), count, 1)
    sim.run()
    return [sim.buf[r]["recv"] for r in range(p)]


def chain3(oracle, op, ty, xs, upto):
    """op3(in1 = x_upto, in2 = op3(in1 = x_{upto-1}, in2 = ... x_0)): the chain written out directly"""
    acc = xs[0].copy()
    for k in range(1, upto + 1):
        x = np.ascontiguousarray(xs[k]).copy()
        out = np.zeros_like(acc)
        oracle.oracle_op_3buff(op, ty, x.ctypes.data, acc.ctypes.data, out.ctypes.data, len(acc))
        acc = out
    return acc
