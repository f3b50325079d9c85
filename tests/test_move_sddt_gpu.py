"""gather(v), scatter(v), allgatherv and alltoall(v) pulling straight OUT of a derived send datatype
(mi355x_*_ddt2, coll_move.cpp; the two-ended row gather k_ddt_rows2_multi of ddt_kernels.hip) on
loopback communicators, one thread per rank.  Every case sets MOVE_SEND_MIN_RUN itself.

Every result is compared byte for byte with two references: a numpy model -- the packed stream of
every piece gathered from the sender's buffer through Layout.inst of the send layout, then placed
(mdl.place) into the receive side -- and the sequence the call replaces: Ddt.pack per piece into dense
bytes, then the _ddt or the plain call.  Receive buffers start as poison with guard bytes either
side; send buffers carry a filler in their gaps and guards, and must be byte-identical afterwards.

Send layouts are the smallest that reach each slot width: vec9 (16), col8 (8, the pieces interleaved
in the sender's memory), vec37 (4), odd3 (1), each into dense bytes and into a receive layout of
another shape, so the run boundaries of the two ends never coincide (a receiver holds the instances
that cover what it is sent; the sender stops inside one).
"""
from __future__ import annotations

import numpy as np
import pytest

import move_ddt_model as mdl
from test_coll_gpu import run_ranks

pytestmark = pytest.mark.gpu

G, POISON, FILL = mdl.GUARD, mdl.POISON, 0x5A
LAYOUTS = {"vec37": mdl.vec37, "vec9": mdl.vec9, "odd3": mdl.odd3, "idx3": mdl.idx3, "contig": mdl.contiguous}


@pytest.fixture(scope="module")
def comms(gpu, pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.Comm.loopback(n, 0)
            for c in made[n]:
                c.set("TIMEOUT_S", 30)      # a rank that fails alone must not leave the others waiting for a day
        return made[n]

    yield get
    for cs in made.values():
        for c in cs:
            c.destroy()


def geometry(name, cnt, rows=50):
    """the layout, the byte displacement of every piece of cnt[q] instances, the bytes they span"""
    if name == "col8":
        ncols = sum(cnt) + 1                          # one spare column: a gap
        first = np.concatenate([[0], np.cumsum(cnt[:-1])])
        return mdl.column(rows, ncols), [int(c) * 8 for c in first], rows * ncols * 8
    lay = LAYOUTS[name]()
    displs, at = [], 0
    for c in cnt:
        displs.append(at)
        at += (lay.span(c) + 15) // 16 * 16 + 32      # pieces 16-byte aligned, 32 filler bytes between
    return lay, displs, at


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Send:
    """one rank's send side: `cnt[r]` instances of the layout for piece r, filler in the gaps and the guards,
    the whole buffer `off` bytes off 16-byte alignment; stream[r] is piece r's packed stream, read back out
    of the buffer through Layout.inst"""

    def __init__(self, torch, name, cnt, seed, off=0):
        self.lay, self.displs, total = geometry(name, cnt)
        self.cnt = list(cnt)
        self.host = np.full(total + 2 * G + 16, FILL, dtype=np.uint8)
        self.lo = G + off
        for r, c in enumerate(cnt):
            idx = self.lo + self.displs[r] + self.lay.offsets(c * self.lay.size)
            self.host[idx] = mdl.payload(seed + r, c * self.lay.size)
        self.stream = [self.host[self.lo + self.displs[r] + self.lay.offsets(c * self.lay.size)].copy()
                       for r, c in enumerate(cnt)]
        self.bytes = [len(s) for s in self.stream]
        self.t = _dev(torch, self.host)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo
        # the dense form of the same side, as the parent's sequence sends it: filled by Ddt.pack
        self.doff = [int(v) for v in np.concatenate([[0], np.cumsum([(b + 15) // 16 * 16 for b in self.bytes[:-1]])])]
        self.dense = torch.full((sum((b + 15) // 16 * 16 for b in self.bytes) + 16,), 0x33, dtype=torch.uint8, device="cuda")

    def pack(self, torch, pkg):
        ddt = self.lay.ddt(pkg)
        for r, c in enumerate(self.cnt):
            if c:
                ddt.pack(c, self.ptr + self.displs[r], 0, self.dense.data_ptr() + self.doff[r], self.bytes[r])
        torch.cuda.synchronize()

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy(), self.host)


class Recv:
    """one rank's receive side for pieces of nbytes[q]: dense bytes (name None) or the instances of a layout
    that cover them; a poisoned device buffer with guards"""

    def __init__(self, torch, name, nbytes, off=0):
        self.name = name
        if name is None:
            self.lay = None
            self.cnt = list(nbytes)
            self.displs = [int(v) for v in np.concatenate([[0], np.cumsum([(b + 15) // 16 * 16 + 16 for b in nbytes[:-1]])])]
            total = sum((b + 15) // 16 * 16 + 16 for b in nbytes)
        else:
            size = geometry(name, [1], rows=33)[0].size      # (a receiver's columns: 33 rows, the senders' 50)
            self.cnt = [-(-b // size) for b in nbytes]
            self.lay, self.displs, total = geometry(name, self.cnt, rows=33)
        self.t = torch.full((total + 2 * G + 16,), POISON, dtype=torch.uint8, device="cuda")
        self.lo = G + off
        self.ptr = self.t.data_ptr() + self.lo
        self.want = np.full(total + 2 * G + 16, POISON, dtype=np.uint8)

    def ddt(self, pkg):
        return self.lay.ddt(pkg) if self.lay else None

    def expect(self, q, stream):
        if self.lay is None:
            self.want[self.lo + self.displs[q]:self.lo + self.displs[q] + len(stream)] = stream
        else:
            mdl.place(self.want, self.lo, self.lay, self.displs[q], stream)

    def got(self):
        return self.t.cpu().numpy()


def _same(rx, ref, what):
    got = rx.got()
    bad = np.nonzero(got != rx.want)[0]
    assert bad.size == 0, f"{what}: differs from the numpy model at byte {bad[0] - rx.lo} (+{bad.size - 1} more)"
    old = ref.got()
    bad = np.nonzero(old != rx.want)[0]
    assert bad.size == 0, f"{what}: the replaced sequence differs from the numpy model at byte {bad[0] - ref.lo}"


def _set_min_run(cs, v):
    for c in cs:
        c.set("MOVE_SEND_MIN_RUN", v)


def _direct(cs):
    return [c.get("MOVE_SEND_DIRECT") for c in cs]


def run_alltoallv(torch, pkg, cs, sname, rname, counts, min_run=1, soff=0, plain=(), what=""):
    """counts[q][r]: instances of its send layout rank q sends to r.  sname / rname: one layout name, or one
    per rank; ranks in `plain` call the plain / _ddt form with the dense bytes of the same side."""
    n = len(cs)
    snames = [sname] * n if isinstance(sname, str) else list(sname)
    rnames = [rname] * n if rname is None or isinstance(rname, str) else list(rname)
    snd = [Send(torch, snames[q], counts[q], 1000 * (q + 1), soff) for q in range(n)]
    rxs = [[Recv(torch, rnames[r], [snd[q].bytes[r] for q in range(n)]) for r in range(n)] for _ in range(2)]
    for r in range(n):
        for q in range(n):
            rxs[0][r].expect(q, snd[q].stream[r])
    for s in snd:
        s.pack(torch, pkg)
    sddt = [snd[q].lay.ddt(pkg) for q in range(n)]
    rddt = [rxs[0][r].ddt(pkg) for r in range(n)]
    _set_min_run(cs, min_run)
    before = _direct(cs)

    def rank(r):
        torch.cuda.set_device(0)
        rx = rxs[0][r]
        if r in plain:
            cs[r].alltoallv_ddt(snd[r].dense.data_ptr(), snd[r].bytes, snd[r].doff, rx.ptr, rddt[r], rx.cnt, rx.displs)
        else:
            cs[r].alltoallv_ddt2(snd[r].ptr, sddt[r], snd[r].cnt, snd[r].displs, rx.ptr, rddt[r], rx.cnt, rx.displs)

    run_ranks(n, rank)
    torch.cuda.synchronize()
    for r in range(n):
        want = 0 if r in plain or not any(snd[r].bytes) else 1
        assert cs[r].get("MOVE_SEND_DIRECT") - before[r] == want, f"{what}: MOVE_SEND_DIRECT on rank {r}"
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv_ddt(
        snd[r].dense.data_ptr(), snd[r].bytes, snd[r].doff, rxs[1][r].ptr, rddt[r], rxs[1][r].cnt, rxs[1][r].displs)))
    torch.cuda.synchronize()
    for r in range(n):
        rxs[1][r].want = rxs[0][r].want
        _same(rxs[0][r], rxs[1][r], f"{what} alltoallv rank {r}")
        assert snd[r].unchanged(), f"{what}: rank {r}'s send buffer changed"


def _counts(n, q):
    return [1 + (3 * q + r) % 5 for r in range(n)]


# the send layout, the receive layout of another shape (run boundaries never coincide: W is the narrower
# end's), MOVE_SEND_MIN_RUN
WIDTHS = [("vec9", "col8", 256), ("col8", "vec9", 8), ("vec37", "vec9", 12), ("odd3", "vec37", 1)]


@pytest.mark.parametrize("dest", ["dense", "layout"])
@pytest.mark.parametrize("sname,rname,min_run", WIDTHS)
def test_every_width(gpu, pkg, comms, sname, rname, min_run, dest):
    """slot widths 16, 8, 4 and 1, each into dense bytes and into a receive layout of another shape"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), sname, rname if dest == "layout" else None, [_counts(n, q) for q in range(n)],
                  min_run=min_run, what=f"{sname}->{rname if dest == 'layout' else 'dense'}")


@pytest.mark.parametrize("rname", [None, "col8"])
def test_three_kinds_of_sender(gpu, pkg, comms, rname):
    """rank 0 sends through vec9, rank 1 calls the plain form with dense bytes, rank 2 sends through vec37:
    every receiver's pieces have source layouts that differ; MOVE_SEND_DIRECT rises on ranks 0 and 2 only"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), ["vec9", "vec37", "vec37"], rname, [_counts(n, q) for q in range(n)], min_run=12,
                  plain=(1,), what="three kinds")


@pytest.mark.parametrize("sname,rname", [("vec9", None), ("col8", "vec37")])
def test_ragged_and_block_looping(gpu, pkg, comms, sname, rname):
    """an empty piece, a one-instance piece beside one of 5000 instances (its blocks loop)"""
    n = 3
    kinds = {"one": 1, "big": 5000, "zero": 0, "few": 3}
    counts = [[kinds[("one", "big", "zero", "few")[(r + 2 * q) % 4]] for r in range(n)] for q in range(n)]
    run_alltoallv(gpu, pkg, comms(n), sname, rname, counts, min_run=8, what=f"ragged {sname}")


@pytest.mark.parametrize("sname,rname", [("vec9", None), ("vec9", "col8")])
def test_send_base_off_alignment(gpu, pkg, comms, sname, rname):
    """the send base 4 bytes past a 16-byte boundary: W drops to 4 for the whole launch"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), sname, rname, [_counts(n, q) for q in range(n)], min_run=8, soff=4,
                  what=f"{sname} base+4")


@pytest.mark.parametrize("n", [2, 8])
def test_alltoallv_sizes(gpu, pkg, comms, n):
    """n = 2; and n = 8 with col8 on both sides: the block transpose"""
    run_alltoallv(gpu, pkg, comms(n), "col8", "col8", [_counts(n, q) for q in range(n)], min_run=8, what=f"transpose n={n}")


def test_fallback_two_passes(gpu, pkg, comms):
    """vec9 into idx3, several runs per block: the rows gathered into the scratch, then unpacked"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), "vec9", "idx3", [_counts(n, q) for q in range(n)], min_run=8, what="vec9->idx3")


def test_gatherv_every_root(gpu, pkg, comms):
    """every rank sends through vec9; the root receives dense bytes (even roots) or into vec37 (odd)"""
    torch, n = gpu, 3
    cs = comms(n)
    _set_min_run(cs, 8)
    for root in range(n):
        cnt = _counts(n, root)
        snd = [Send(torch, "vec9", [cnt[q]], 2000 + 10 * root + q) for q in range(n)]
        rname = "vec37" if root % 2 else None
        rxs = [Recv(torch, rname, [snd[q].bytes[0] for q in range(n)]) for _ in range(2)]
        for q in range(n):
            rxs[0].expect(q, snd[q].stream[0])
            snd[q].pack(torch, pkg)
        sddt, rddt = snd[0].lay.ddt(pkg), rxs[0].ddt(pkg)
        before = _direct(cs)
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv_ddt2(
            snd[r].ptr, sddt, cnt[r], rxs[0].ptr if r == root else None, rddt if r == root else None,
            rxs[0].cnt if r == root else None, rxs[0].displs if r == root else None, root)))
        assert [a - b for a, b in zip(_direct(cs), before)] == [1] * n
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv_ddt(
            snd[r].dense.data_ptr(), snd[r].bytes[0], rxs[1].ptr if r == root else None, rddt if r == root else None,
            rxs[1].cnt if r == root else None, rxs[1].displs if r == root else None, root)))
        torch.cuda.synchronize()
        rxs[1].want = rxs[0].want
        _same(rxs[0], rxs[1], f"gatherv root {root}")
        assert all(s.unchanged() for s in snd)


def test_scatterv_every_root(gpu, pkg, comms):
    """the root alone has a send side (col8, the pieces interleaved): the others pass no layout; receivers
    take dense bytes (even ranks) or vec9 (odd)"""
    torch, n = gpu, 3
    cs = comms(n)
    _set_min_run(cs, 8)
    for root in range(n):
        snd = Send(torch, "col8", _counts(n, root), 3000 + 10 * root)
        snd.pack(torch, pkg)
        rxs = [[Recv(torch, "vec9" if r % 2 else None, [snd.bytes[r]]) for r in range(n)] for _ in range(2)]
        for r in range(n):
            rxs[0][r].expect(0, snd.stream[r])
        sddt = snd.lay.ddt(pkg)
        rddt = [rxs[0][r].ddt(pkg) for r in range(n)]
        before = _direct(cs)
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv_ddt2(
            snd.ptr if r == root else None, sddt if r == root else None, snd.cnt if r == root else None,
            snd.displs if r == root else None, rxs[0][r].ptr, rddt[r], rxs[0][r].cnt[0], root)))
        assert [a - b for a, b in zip(_direct(cs), before)] == [1 if r == root else 0 for r in range(n)]
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv_ddt(
            snd.dense.data_ptr() if r == root else None, snd.bytes if r == root else None,
            snd.doff if r == root else None, rxs[1][r].ptr, rddt[r], rxs[1][r].cnt[0], root)))
        torch.cuda.synchronize()
        for r in range(n):
            rxs[1][r].want = rxs[0][r].want
            _same(rxs[0][r], rxs[1][r], f"scatterv root {root} rank {r}")
        assert snd.unchanged()


@pytest.mark.parametrize("rname", [None, "vec37"])
def test_allgatherv(gpu, pkg, comms, rname):
    """allgatherv publishes no counts: a receiver's piece holds exactly what its sender sends, so into vec37
    (444 bytes) the senders send multiples of 37 instances of vec9 (2304 bytes) = 192 of vec37"""
    torch, n = gpu, 3
    cs = comms(n)
    _set_min_run(cs, 8)
    cnt = [37, 74, 37] if rname else _counts(n, 1)
    snd = [Send(torch, "vec9", [cnt[q]], 4000 + q) for q in range(n)]
    assert rname is None or all(s.bytes[0] % 444 == 0 for s in snd)
    rxs = [[Recv(torch, rname, [snd[q].bytes[0] for q in range(n)]) for _ in range(n)] for _ in range(2)]
    for q in range(n):
        snd[q].pack(torch, pkg)
        for r in range(n):
            rxs[0][r].expect(q, snd[q].stream[0])
    sddt, rddt = snd[0].lay.ddt(pkg), rxs[0][0].ddt(pkg)
    before = _direct(cs)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv_ddt2(
        snd[r].ptr, sddt, cnt[r], rxs[0][r].ptr, rddt, rxs[0][r].cnt, rxs[0][r].displs)))
    assert [a - b for a, b in zip(_direct(cs), before)] == [1] * n
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv_ddt(
        snd[r].dense.data_ptr(), snd[r].bytes[0], rxs[1][r].ptr, rddt, rxs[1][r].cnt, rxs[1][r].displs)))
    torch.cuda.synchronize()
    for r in range(n):
        rxs[1][r].want = rxs[0][r].want
        _same(rxs[0][r], rxs[1][r], f"allgatherv rank {r}")
    assert all(s.unchanged() for s in snd)


def test_truncation_is_refused(gpu, pkg, comms):
    """a receiver whose layout holds fewer bytes than a direct sender sends: MI355X_ERR_TRUNCATE, as in the
    plain form (every rank is short, so every rank returns after the meeting point)"""
    torch, n = gpu, 3
    cs = comms(n)
    _set_min_run(cs, 8)
    snd = [Send(torch, "vec9", [2] * n, 5000 + q) for q in range(n)]
    rx = [Recv(torch, "vec37", [snd[q].bytes[r] for q in range(n)]) for r in range(n)]
    sddt, rddt = snd[0].lay.ddt(pkg), rx[0].ddt(pkg)
    seen = []

    def rank(r):
        torch.cuda.set_device(0)
        short = [c - 1 for c in rx[r].cnt]
        with pytest.raises(pkg.MI355XError, match="MI355X_ERR_TRUNCATE"):
            cs[r].alltoallv_ddt2(snd[r].ptr, sddt, snd[r].cnt, snd[r].displs, rx[r].ptr, rddt, short, rx[r].displs)
        seen.append(r)

    run_ranks(n, rank)
    assert sorted(seen) == list(range(n))
    torch.cuda.synchronize()
    for r in range(n):
        assert bool((rx[r].t == POISON).all()) and snd[r].unchanged()
    run_alltoallv(torch, pkg, cs, "vec9", "vec37", [[1] * n] * n, min_run=8, what="after the refusals")


@pytest.mark.parametrize("case", ["idx3", "short_run", "never", "in_place"])
def test_not_eligible_is_unsupported(gpu, pkg, comms, case):
    """MI355X_ERR_UNSUPPORTED before the rank meets anybody: nothing written, MOVE_SEND_DIRECT stays, and
    mi355x_move_send_direct_ok says so too"""
    torch, n = gpu, 3
    cs = comms(n)
    sname = "idx3" if case == "idx3" else "vec37"
    _set_min_run(cs, {"idx3": 1, "short_run": 13, "never": 0, "in_place": 1}[case])
    snd = [Send(torch, sname, [2] * n, 6000 + q) for q in range(n)]
    rx = [Recv(torch, None, [snd[q].bytes[r] for q in range(n)]) for r in range(n)]
    sddt = snd[0].lay.ddt(pkg)
    before = _direct(cs)
    seen = []

    def rank(r):
        torch.cuda.set_device(0)
        assert cs[r].move_send_direct_ok(sddt, snd[r].cnt) == (case == "in_place")   # (the rule's own in-place clause
        with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):        # is the call's: sbuf NULL)
            if case == "in_place":
                cs[r].alltoallv_ddt2(None, sddt, None, None, rx[r].ptr, None, rx[r].cnt, rx[r].displs)
            else:
                cs[r].alltoallv_ddt2(snd[r].ptr, sddt, snd[r].cnt, snd[r].displs, rx[r].ptr, None, rx[r].cnt, rx[r].displs)
        if case == "in_place":
            with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):
                cs[r].allgatherv_ddt2(None, sddt, 2, rx[r].ptr, None, rx[r].cnt, rx[r].displs)
        seen.append(r)

    run_ranks(n, rank)
    assert sorted(seen) == list(range(n))
    torch.cuda.synchronize()
    assert _direct(cs) == before
    for r in range(n):
        assert bool((rx[r].t == POISON).all()) and snd[r].unchanged()
    if case == "short_run":      # the other side of MIN_RUN: the run itself is published
        _set_min_run(cs, 12)
        assert cs[0].move_send_direct_ok(sddt, snd[0].cnt)
    run_alltoallv(torch, pkg, cs, "vec37", None, [[1] * n] * n, min_run=12, what="after the refusals")


def test_gap_free_send_layout_is_the_plain_call(gpu, pkg, comms):
    """contig as the send layout: the plain call, exact, MOVE_SEND_DIRECT stays"""
    torch, n = gpu, 3
    cs = comms(n)
    _set_min_run(cs, 1)
    snd = [Send(torch, "contig", _counts(n, q), 7000 + q) for q in range(n)]
    rx = [Recv(torch, "vec37", [snd[q].bytes[r] for q in range(n)]) for r in range(n)]
    for r in range(n):
        for q in range(n):
            rx[r].expect(q, snd[q].stream[r])
    sddt, rddt = snd[0].lay.ddt(pkg), rx[0].ddt(pkg)
    assert not cs[0].move_send_direct_ok(sddt, snd[0].cnt)
    before = _direct(cs)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv_ddt2(
        snd[r].ptr, sddt, snd[r].cnt, snd[r].displs, rx[r].ptr, rddt, rx[r].cnt, rx[r].displs)))
    torch.cuda.synchronize()
    assert _direct(cs) == before
    for r in range(n):
        assert np.array_equal(rx[r].got(), rx[r].want), f"rank {r}"
        assert snd[r].unchanged()


def test_knobs(gpu, pkg, comms):
    c = comms(2)[0]
    assert pkg.KNOB["MOVE_SEND_DIRECT"] == 47 and pkg.KNOB["MOVE_SEND_MIN_RUN"] == 48
    with pytest.raises(pkg.MI355XError):
        c.set("MOVE_SEND_DIRECT", 0)
    c.set("MOVE_SEND_MIN_RUN", 4096)
    assert c.get("MOVE_SEND_MIN_RUN") == 4096
    with pytest.raises(pkg.MI355XError, match="move_send_min_run out of range"):
        c.set("MOVE_SEND_MIN_RUN", -1)
    assert c.get("MOVE_SEND_MIN_RUN") == 4096
