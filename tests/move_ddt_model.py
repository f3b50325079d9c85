"""The receive layouts of tests/test_move_ddt_gpu.py and tests/move_ddt_worker.py, each written out
twice: as the GPU convertor's Ddt and as a numpy type map (the byte offsets of one instance in packed
order), so a placement can be computed without the code under test.

A layout here is one or more runs (disp, len) per block, nblk blocks `stride` bytes apart, instances
`extent` bytes apart -- the terms of include/mi355x_rt.h's mi355x_ddt_create.
"""
from __future__ import annotations

import numpy as np

POISON = 0xA5
GUARD = 64          # guard bytes either side of a receive buffer (a multiple of 16)


class Layout:
    def __init__(self, name, runs, nblk, stride, extent, make):
        self.name, self.runs, self.nblk, self.stride, self.extent = name, runs, nblk, stride, extent
        self._make = make
        one = np.concatenate([np.arange(d, d + ln, dtype=np.int64) for d, ln in runs])
        self.inst = (np.arange(nblk, dtype=np.int64)[:, None] * stride + one[None, :]).ravel()
        self.size = int(self.inst.size)
        self.run = runs[0][1]

    def ddt(self, pkg):
        return self._make(pkg)

    def offsets(self, nbytes):
        """memory offsets (from the piece's base) of the first nbytes of the piece's packed stream"""
        k = -(-nbytes // self.size) if self.size else 0
        return (np.arange(k, dtype=np.int64)[:, None] * self.extent + self.inst[None, :]).ravel()[:nbytes]

    def span(self, count):
        """bytes from the piece's base to the end of its last instance"""
        return 0 if count == 0 else (count - 1) * self.extent + int(self.inst.max()) + 1


def vec37():   # vector(37, 3, 5) of floats: 12-byte runs, slot width 4
    return Layout("vec37", [(0, 12)], 37, 20, (36 * 5 + 3) * 4, lambda pkg: pkg.Ddt.vector(37, 3, 5, 4))


def vec9():    # vector(9, 64, 128) of floats: 256-byte runs, slot width 16; an instance is 144 slots
    return Layout("vec9", [(0, 256)], 9, 512, (8 * 128 + 64) * 4, lambda pkg: pkg.Ddt.vector(9, 64, 128, 4))


def column(rows, ncols):   # a column of doubles in a rows x ncols matrix, resized to one element: width 8
    return Layout("col8", [(0, 8)], rows, ncols * 8, 8, lambda pkg: pkg.Ddt.runs([0], [8], rows, ncols * 8, 8))


def odd3():    # 3-byte runs at stride 7: slot width 1
    return Layout("odd3", [(0, 3)], 11, 7, 77, lambda pkg: pkg.Ddt.runs([0], [3], 11, 7, 77))


def idx3():    # indexed, runs of 4, 12 and 8 bytes: several runs per block, the per-piece path
    return Layout("idx3", [(0, 4), (8, 12), (28, 8)], 1, 0, 36, lambda pkg: pkg.Ddt.indexed([1, 3, 2], [0, 2, 7], 4))


def contiguous():   # 16 floats, no gap: the plain call
    return Layout("contig", [(0, 64)], 1, 0, 64, lambda pkg: pkg.Ddt.vector(1, 16, 16, 4))


def place(want, base, layout, displ, data):
    """numpy model: the packed bytes `data` of one piece into want (uint8) laid at base + displ"""
    want[base + displ + layout.offsets(len(data))] = data


def payload(seed, nbytes):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
