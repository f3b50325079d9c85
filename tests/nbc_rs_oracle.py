"""Test-side reference for coll/libnbc's MPI_Ireduce_scatter (vector counts), on the message-passing
simulator of tests/nbc_oracle.py.

The schedule is restated from nbc_ireduce_scatter.c:84-152: `tmp` and `red` are of the whole vector
(the two halves of the handle's tmpbuf), the binomial reduce to rank 0 runs over the total count with
every step NBC_Sched_op(red, sendbuf or red, tmp), then rank 0 sends red[offset_r : offset_r +
recvcounts[r]] to rank r and copies its own block, and every other rank receives recvcounts[r]
elements at the start of its recvbuf.  With MPI_IN_PLACE sendbuf is recvbuf (NBC_IN_PLACE).
"""
from __future__ import annotations

import numpy as np

import nbc_oracle as nbc

# the count vectors the tests share: the smallest that still exercise the block arithmetic
VECTORS = ("equal", "ragged", "holes", "one_owner", "empty")


def counts_of(kind: str, n: int) -> list[int]:
    if kind == "equal":
        return [5] * n
    if kind == "ragged":            # every block but the first starts off a 16-byte boundary
        return [1 + 37 * r for r in range(n)]
    if kind == "holes":
        c = counts_of("ragged", n)
        c[0] = c[n - 1] = 0
        return c
    if kind == "one_owner":
        return [0] * (n - 1) + [4099]
    assert kind == "empty"
    return [0] * n


def ireduce_scatter(oracle, op, ty, xs, rcounts, inplace=False):
    """returns (every rank's recvbuf[:rcounts[r]], BINOMIAL)"""
    p, count = len(xs), len(xs[0])
    assert count == sum(rcounts) and len(rcounts) == p and p > 1
    sim = nbc.Sim(oracle, op, ty, p)
    for r in range(p):
        b = sim.buf[r]
        b["recv"] = xs[r].copy() if inplace else np.zeros(rcounts[r], dtype=xs[r].dtype)
        b["send"] = b["recv"] if inplace else xs[r].copy()
        b["tmp"] = np.zeros_like(xs[r])
        b["red"] = np.zeros_like(xs[r])
        nbc._binomial_up(sim, r, p, 0, count, "red")
        sim.barrier(r)
        if r != 0:
            sim.recv(r, ("recv", 0), rcounts[r], 0)
        else:
            offset = 0
            for q in range(1, p):
                offset += rcounts[q - 1]
                sim.send(r, ("red", offset), rcounts[q], q)
            sim.copy(r, ("red", 0), ("recv", 0), rcounts[0])
    sim.run()
    return [sim.buf[r]["recv"][:rcounts[r]].copy() for r in range(p)], nbc.BINOMIAL
