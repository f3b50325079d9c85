"""Guarded device buffers and knob scopes shared by the loopback suites (test_coll_wide_gpu.py) and
the multi-process worker (ipc_worker.py::offalign).  No pytest import: a worker process uses it."""
from __future__ import annotations

import numpy as np

GUARD = 64          # bytes of 0xA5 in front of and behind every device buffer


class Buf:
    """`count` elements of device memory `shift` bytes past a 16-byte boundary, between two guards"""

    def __init__(self, torch, like: np.ndarray, count: int, shift: int = 0, init: np.ndarray | None = None):
        self.like, self.count, self.off = like, count, GUARD + shift
        self.nbytes = count * like.dtype.itemsize
        host = np.full(self.off + self.nbytes + GUARD, 0xA5, dtype=np.uint8)
        host[self.off:self.off + self.nbytes] = 0 if init is None else np.ascontiguousarray(init).view(np.uint8).reshape(-1)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.off

    def get(self, count: int | None = None) -> np.ndarray:
        nb = (self.count if count is None else count) * self.like.dtype.itemsize
        return self.t[self.off:self.off + nb].cpu().numpy().view(self.like.dtype).copy()

    def raw(self) -> np.ndarray:
        """the payload's bytes as they are in device memory (get() goes through numpy's copy() of the
        element type, which leaves a pair type's padding bytes unset)"""
        return self.t[self.off:self.off + self.nbytes].cpu().numpy()

    def holds(self, a: np.ndarray | None) -> bool:
        """every byte equal to those of the host array it was filled from (None: still zero), compared
        as raw bytes: numpy's copy() and zeros_like() of a pair type leave the padding bytes unset"""
        want = np.zeros(self.nbytes, dtype=np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return bool((self.t[self.off:self.off + self.nbytes].cpu().numpy() == want).all())

    def guards_intact(self) -> bool:
        front, back = self.t[:self.off].cpu().numpy(), self.t[self.off + self.nbytes:].cpu().numpy()
        return bool((front == 0xA5).all() and (back == 0xA5).all())


class knobs:
    """set knobs on every rank of a communicator; give the previous values back on the way out"""

    def __init__(self, cs, **kv):
        self.cs, self.kv = cs, kv

    def __enter__(self):
        self.old = {k: self.cs[0].get(k) for k in self.kv}
        for c in self.cs:
            for k, v in self.kv.items():
                c.set(k, v)

    def __exit__(self, *exc):
        for c in self.cs:
            for k, v in self.old.items():
                c.set(k, v)
