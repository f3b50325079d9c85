"""gather(v), scatter(v), allgatherv and alltoall(v) pulling straight through row layouts of TWO levels --
the pencil or slab of a 3-D array, a 3-D subarray, an hvector of vectors -- on either side
(mi355x_*_ddt2 / _ddt under MOVE_ROW_LEVELS = 2; row_levels_view of ddt_rows_plan.hpp, the level
parameter of k_ddt_rows2_multi in ddt_kernels.hip) on loopback communicators, one thread per rank.  Every
case sets MOVE_ROW_LEVELS and MOVE_SEND_MIN_RUN itself.

Every result is compared byte for byte with the numpy model (move_ddt_model.Layout takes several runs per
block) and, for send layouts, with the sequence the call replaces: Ddt.pack per piece into dense bytes,
then the _ddt or the plain call under MOVE_ROW_LEVELS = 1.  Receive buffers start as poison between guard
bytes; send buffers carry a filler in their gaps and must be byte-identical afterwards.

The layouts are the smallest that reach each slot width with both levels live and counts that share no
factor (sub16: an instance is 45 slots and a row 3, so the lanes of one wave cross rows and groups), each
into dense bytes and into a receive layout of another shape, so the run, row and group boundaries of the
two ends never coincide.
"""
from __future__ import annotations

import numpy as np
import pytest

import move_ddt_model as mdl
import test_move_sddt_gpu as sd
from test_coll_gpu import run_ranks

pytestmark = pytest.mark.gpu

G, POISON, FILL = mdl.GUARD, mdl.POISON, 0x5A


def _runs(name, disps, run, nblk, stride, extent):
    return mdl.Layout(name, [(d, run) for d in disps], nblk, stride, extent,
                      lambda pkg: pkg.Ddt.runs(list(disps), [run] * len(disps), nblk, stride, extent))


def sub16():   # 3 rows of 48 B at 80 B, 5 groups at 400 B: slot width 16, an instance is 45 slots
    return _runs("sub16", [0, 80, 160], 48, 5, 400, 2000)


def flat():    # the same bytes as ONE block of 15 unrolled runs: a description whose top level is no loop
    return _runs("flat", [(r % 3) * 80 + (r // 3) * 400 for r in range(15)], 48, 1, 0, 2000)


def sub8(C):   # pencils of doubles in a 16 x C array resized to one element: slot width 8, pieces interleave
    return _runs("sub8", [0, 8 * C, 16 * C], 8, 4, 32 * C, 8)


def sub4():    # 3 rows of 12 B at 20 B, 7 groups at 68 B: slot width 4
    return _runs("sub4", [0, 20, 40], 12, 7, 68, 476)


def sub1():    # 2 rows of 3 B at 7 B, 5 groups at 17 B: slot width 1
    return _runs("sub1", [0, 7], 3, 5, 17, 85)


def merge():   # 3 rows at 80 B, 5 groups at 240 B: the groups continue the rows -- 15 rows, one level
    return _runs("merge", [0, 80, 160], 48, 5, 240, 2000)


def vec15():   # ... the 15-row vector itself, one run per block
    return _runs("vec15", [0], 48, 15, 80, 2000)


def three():   # a two-level run table times two blocks that do not continue it: three levels, a run list
    return _runs("three", [0, 80, 160, 400, 480, 560], 48, 2, 1000, 2400)


PLANES = {"sub16": sub16, "flat": flat, "sub4": sub4, "sub1": sub1, "merge": merge, "vec15": vec15, "three": three}


def geometry(name, cnt, rows=50):
    """test_move_sddt_gpu.geometry with the layouts of this file"""
    if name == "sub8":
        C = sum(cnt) + 1                              # one spare column: a gap
        first = np.concatenate([[0], np.cumsum(cnt[:-1])])
        return sub8(C), [int(c) * 8 for c in first], 128 * C
    if name not in PLANES:
        return sd.geometry(name, cnt, rows)
    lay = PLANES[name]()
    displs, at = [], 0
    for c in cnt:
        displs.append(at)
        at += (lay.span(c) + 15) // 16 * 16 + 32      # pieces 16-byte aligned, 32 filler bytes between
    return lay, displs, at


class Send(sd.Send):
    """test_move_sddt_gpu.Send over this file's geometry"""

    def __init__(self, torch, name, cnt, seed, off=0):
        self.lay, self.displs, total = geometry(name, cnt)
        self.cnt = list(cnt)
        self.host = np.full(total + 2 * G + 16, FILL, dtype=np.uint8)
        self.lo = G + off
        for r, c in enumerate(cnt):
            self.host[self.lo + self.displs[r] + self.lay.offsets(c * self.lay.size)] = mdl.payload(seed + r, c * self.lay.size)
        self.stream = [self.host[self.lo + self.displs[r] + self.lay.offsets(c * self.lay.size)].copy()
                       for r, c in enumerate(cnt)]
        self.bytes = [len(s) for s in self.stream]
        self.t = sd._dev(torch, self.host)
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo
        pad = [(b + 15) // 16 * 16 for b in self.bytes]
        self.doff = [int(v) for v in np.concatenate([[0], np.cumsum(pad[:-1])])]
        self.dense = torch.full((sum(pad) + 16,), 0x33, dtype=torch.uint8, device="cuda")


class Recv(sd.Recv):
    """test_move_sddt_gpu.Recv over this file's geometry"""

    def __init__(self, torch, name, nbytes, off=0):
        self.name = name
        if name is None:
            self.lay = None
            self.cnt = list(nbytes)
            self.displs = [int(v) for v in np.concatenate([[0], np.cumsum([(b + 15) // 16 * 16 + 16 for b in nbytes[:-1]])])]
            total = sum((b + 15) // 16 * 16 + 16 for b in nbytes)
        else:
            size = geometry(name, [1], rows=33)[0].size
            self.cnt = [-(-b // size) for b in nbytes]
            self.lay, self.displs, total = geometry(name, self.cnt, rows=33)
        self.t = torch.full((total + 2 * G + 16,), POISON, dtype=torch.uint8, device="cuda")
        self.lo = G + off
        self.ptr = self.t.data_ptr() + self.lo
        self.want = np.full(total + 2 * G + 16, POISON, dtype=np.uint8)


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


def _knobs(cs, levels, min_run=1):
    for c in cs:
        c.set("MOVE_ROW_LEVELS", levels)
        c.set("MOVE_SEND_MIN_RUN", min_run)


def _get(cs, knob):
    return [c.get(knob) for c in cs]


def _counts(n, q):
    return [1 + (3 * q + r) % 5 for r in range(n)]


def run_alltoallv(torch, pkg, cs, sname, rname, counts, min_run=1, soff=0, plain=(), what=""):
    """test_move_sddt_gpu.run_alltoallv under MOVE_ROW_LEVELS = 2, the replaced sequence under 1"""
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
    _knobs(cs, 2, min_run)
    before = _get(cs, "MOVE_SEND_DIRECT")

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
    _knobs(cs, 1, min_run)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv_ddt(
        snd[r].dense.data_ptr(), snd[r].bytes, snd[r].doff, rxs[1][r].ptr, rddt[r], rxs[1][r].cnt, rxs[1][r].displs)))
    torch.cuda.synchronize()
    for r in range(n):
        rxs[1][r].want = rxs[0][r].want
        sd._same(rxs[0][r], rxs[1][r], f"{what} alltoallv rank {r}")
        assert snd[r].unchanged(), f"{what}: rank {r}'s send buffer changed"
    return rxs[0]


def test_row_levels(pkg):
    """how the movement collectives read each layout of this file (host only)"""
    want = {"sub16": 2, "flat": 2, "sub4": 2, "sub1": 2, "merge": 1, "vec15": 1, "three": 0}
    for name, lev in want.items():
        assert PLANES[name]().ddt(pkg).row_levels() == lev, name
    assert sub8(7).ddt(pkg).row_levels() == 2
    assert mdl.vec9().ddt(pkg).row_levels() == 1 and mdl.column(50, 9).ddt(pkg).row_levels() == 1
    assert mdl.idx3().ddt(pkg).row_levels() == 0
    assert pkg.Ddt.runs([0, 8, 16, 24], [4] * 4, 1, 0, 36).row_levels() == 1     # one block of equally spaced runs
    assert pkg.Ddt.runs([0, 8, 17, 24], [4] * 4, 1, 0, 36).row_levels() == 0     # one displacement off by one
    assert np.array_equal(flat().inst, sub16().inst) and np.array_equal(merge().inst, vec15().inst)


# the send layout, the receive layout of another shape (W is the narrower end's), MOVE_SEND_MIN_RUN
WIDTHS = [("sub16", "sub8", 48), ("sub8", "sub16", 8), ("sub4", "sub16", 12), ("sub1", "sub4", 3)]


@pytest.mark.parametrize("dest", ["dense", "layout"])
@pytest.mark.parametrize("sname,rname,min_run", WIDTHS)
def test_every_width(gpu, pkg, comms, sname, rname, min_run, dest):
    """slot widths 16, 8, 4 and 1 with two levels on the send side, into dense bytes and into a two-level
    receive layout of another shape; the stream ends inside a row"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), sname, rname if dest == "layout" else None, [_counts(n, q) for q in range(n)],
                  min_run=min_run, what=f"{sname}->{rname if dest == 'layout' else 'dense'}")


@pytest.mark.parametrize("sname,rname", [("vec9", "sub16"), ("sub16", "col8")])
def test_mixed_with_one_level(gpu, pkg, comms, sname, rname):
    """one end of one level, the other of two"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), sname, rname, [_counts(n, q) for q in range(n)], min_run=8, what=f"{sname}->{rname}")


def test_three_kinds_of_sender(gpu, pkg, comms):
    """rank 0 sends through sub16, rank 1 calls the plain form with dense bytes, rank 2 sends through vec37;
    every rank receives into sub4: MOVE_SEND_DIRECT rises on ranks 0 and 2 only"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), ["sub16", "vec37", "vec37"], "sub4", [_counts(n, q) for q in range(n)], min_run=12,
                  plain=(1,), what="three kinds")


@pytest.mark.parametrize("rname", [None, "sub4"])
def test_ragged_and_block_looping(gpu, pkg, comms, rname):
    """an empty piece, pieces of 1 and 3 instances beside one of 5000 (its blocks loop)"""
    n = 3
    kinds = {"one": 1, "big": 5000, "zero": 0, "few": 3}
    counts = [[kinds[("one", "big", "zero", "few")[(r + 2 * q) % 4]] for r in range(n)] for q in range(n)]
    run_alltoallv(gpu, pkg, comms(n), "sub16", rname, counts, min_run=8, what="ragged sub16")


@pytest.mark.parametrize("rname", [None, "sub8"])
def test_send_base_off_alignment(gpu, pkg, comms, rname):
    """the send base 4 bytes past a 16-byte boundary: W drops to 4 for the whole launch"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), "sub16", rname, [_counts(n, q) for q in range(n)], min_run=8, soff=4, what="sub16 base+4")


@pytest.mark.parametrize("n", [2, 8])
def test_alltoallv_sizes(gpu, pkg, comms, n):
    """n = 2 and n = 8 with sub8 on both sides: the transpose of pencils"""
    run_alltoallv(gpu, pkg, comms(n), "sub8", "sub8", [_counts(n, q) for q in range(n)], min_run=8, what=f"pencils n={n}")


def test_flat_is_sub16(gpu, pkg, comms):
    """ONE block of 15 unrolled runs is read as the same two levels: published, received in one launch, and
    the bytes are sub16's"""
    torch, n = gpu, 3
    cs = comms(n)
    counts = [_counts(n, q) for q in range(n)]
    a = run_alltoallv(torch, pkg, cs, "flat", "sub4", counts, min_run=48, what="flat->sub4")
    b = run_alltoallv(torch, pkg, cs, "sub16", "sub4", counts, min_run=48, what="sub16->sub4")
    for r in range(n):
        assert np.array_equal(a[r].got(), b[r].got())
    a = run_alltoallv(torch, pkg, cs, "sub8", "flat", counts, min_run=8, what="sub8->flat")
    b = run_alltoallv(torch, pkg, cs, "sub8", "sub16", counts, min_run=8, what="sub8->sub16")
    for r in range(n):
        assert np.array_equal(a[r].got(), b[r].got())


def test_merge_is_the_vector(gpu, pkg, comms):
    """groups that continue the rows are one level: published and served like the 15-row vector"""
    torch, n = gpu, 3
    cs = comms(n)
    counts = [_counts(n, q) for q in range(n)]
    a = run_alltoallv(torch, pkg, cs, "merge", "sub4", counts, min_run=48, what="merge->sub4")
    b = run_alltoallv(torch, pkg, cs, "vec15", "sub4", counts, min_run=48, what="vec15->sub4")
    for r in range(n):
        assert np.array_equal(a[r].got(), b[r].got())
    a = run_alltoallv(torch, pkg, cs, "sub4", "merge", counts, min_run=12, what="sub4->merge")
    b = run_alltoallv(torch, pkg, cs, "sub4", "vec15", counts, min_run=12, what="sub4->vec15")
    for r in range(n):
        assert np.array_equal(a[r].got(), b[r].got())


def test_fallback_two_passes(gpu, pkg, comms):
    """sub16 into idx3, a run list: the rows gathered into the scratch, then unpacked"""
    n = 3
    run_alltoallv(gpu, pkg, comms(n), "sub16", "idx3", [_counts(n, q) for q in range(n)], min_run=8, what="sub16->idx3")


def test_gatherv_every_root(gpu, pkg, comms):
    """every rank sends through sub16; the root receives dense bytes (even roots) or into sub4 (odd)"""
    torch, n = gpu, 3
    cs = comms(n)
    for root in range(n):
        cnt = _counts(n, root)
        snd = [Send(torch, "sub16", [cnt[q]], 2000 + 10 * root + q) for q in range(n)]
        rname = "sub4" if root % 2 else None
        rxs = [Recv(torch, rname, [snd[q].bytes[0] for q in range(n)]) for _ in range(2)]
        for q in range(n):
            rxs[0].expect(q, snd[q].stream[0])
            snd[q].pack(torch, pkg)
        sddt, rddt = snd[0].lay.ddt(pkg), rxs[0].ddt(pkg)
        _knobs(cs, 2, 8)
        before = _get(cs, "MOVE_SEND_DIRECT")
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv_ddt2(
            snd[r].ptr, sddt, cnt[r], rxs[0].ptr if r == root else None, rddt if r == root else None,
            rxs[0].cnt if r == root else None, rxs[0].displs if r == root else None, root)))
        assert [a - b for a, b in zip(_get(cs, "MOVE_SEND_DIRECT"), before)] == [1] * n
        _knobs(cs, 1, 8)
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv_ddt(
            snd[r].dense.data_ptr(), snd[r].bytes[0], rxs[1].ptr if r == root else None, rddt if r == root else None,
            rxs[1].cnt if r == root else None, rxs[1].displs if r == root else None, root)))
        torch.cuda.synchronize()
        rxs[1].want = rxs[0].want
        sd._same(rxs[0], rxs[1], f"gatherv root {root}")
        assert all(s.unchanged() for s in snd)


def test_scatterv_every_root(gpu, pkg, comms):
    """the root alone has a send side (sub8, the pieces interleaved); receivers take dense bytes (even ranks)
    or sub16 (odd)"""
    torch, n = gpu, 3
    cs = comms(n)
    for root in range(n):
        snd = Send(torch, "sub8", _counts(n, root), 3000 + 10 * root)
        snd.pack(torch, pkg)
        rxs = [[Recv(torch, "sub16" if r % 2 else None, [snd.bytes[r]]) for r in range(n)] for _ in range(2)]
        for r in range(n):
            rxs[0][r].expect(0, snd.stream[r])
        sddt = snd.lay.ddt(pkg)
        rddt = [rxs[0][r].ddt(pkg) for r in range(n)]
        _knobs(cs, 2, 8)
        before = _get(cs, "MOVE_SEND_DIRECT")
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv_ddt2(
            snd.ptr if r == root else None, sddt if r == root else None, snd.cnt if r == root else None,
            snd.displs if r == root else None, rxs[0][r].ptr, rddt[r], rxs[0][r].cnt[0], root)))
        assert [a - b for a, b in zip(_get(cs, "MOVE_SEND_DIRECT"), before)] == [1 if r == root else 0 for r in range(n)]
        _knobs(cs, 1, 8)
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv_ddt(
            snd.dense.data_ptr() if r == root else None, snd.bytes if r == root else None,
            snd.doff if r == root else None, rxs[1][r].ptr, rddt[r], rxs[1][r].cnt[0], root)))
        torch.cuda.synchronize()
        for r in range(n):
            rxs[1][r].want = rxs[0][r].want
            sd._same(rxs[0][r], rxs[1][r], f"scatterv root {root} rank {r}")
        assert snd.unchanged()


def test_allgatherv(gpu, pkg, comms):
    """allgatherv publishes no counts, so a piece holds exactly what its sender sends: 7 instances of sub16
    (5040 bytes) are 20 of sub4"""
    torch, n = gpu, 3
    cs = comms(n)
    cnt = [7, 14, 7]
    snd = [Send(torch, "sub16", [cnt[q]], 4000 + q) for q in range(n)]
    assert all(s.bytes[0] % 5040 == 0 for s in snd) and sub4().size * 20 == 5040
    rxs = [[Recv(torch, "sub4", [snd[q].bytes[0] for q in range(n)]) for _ in range(n)] for _ in range(2)]
    for q in range(n):
        snd[q].pack(torch, pkg)
        for r in range(n):
            rxs[0][r].expect(q, snd[q].stream[0])
    sddt, rddt = snd[0].lay.ddt(pkg), rxs[0][0].ddt(pkg)
    _knobs(cs, 2, 8)
    before = _get(cs, "MOVE_SEND_DIRECT")
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv_ddt2(
        snd[r].ptr, sddt, cnt[r], rxs[0][r].ptr, rddt, rxs[0][r].cnt, rxs[0][r].displs)))
    assert [a - b for a, b in zip(_get(cs, "MOVE_SEND_DIRECT"), before)] == [1] * n
    _knobs(cs, 1, 8)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv_ddt(
        snd[r].dense.data_ptr(), snd[r].bytes[0], rxs[1][r].ptr, rddt, rxs[1][r].cnt, rxs[1][r].displs)))
    torch.cuda.synchronize()
    for r in range(n):
        rxs[1][r].want = rxs[0][r].want
        sd._same(rxs[0][r], rxs[1][r], f"allgatherv rank {r}")
    assert all(s.unchanged() for s in snd)


def test_receive_only_is_one_launch(gpu, pkg, comms):
    """alltoallv_ddt with dense senders into sub16: one launch for all peers (MOVE_FUSED + 1,
    MOVE_PULL_LAUNCHES + 1 per rank); under MOVE_ROW_LEVELS = 1 the same bytes from n launches"""
    torch, n = gpu, 3
    cs = comms(n)
    snd = [Send(torch, "vec9", _counts(n, q), 8000 + q) for q in range(n)]
    for s in snd:
        s.pack(torch, pkg)
    rxs = [[Recv(torch, "sub16", [snd[q].bytes[r] for q in range(n)]) for r in range(n)] for _ in range(2)]
    for r in range(n):
        for q in range(n):
            rxs[0][r].expect(q, snd[q].stream[r])
    rddt = rxs[0][0].ddt(pkg)
    for k, (levels, launches) in enumerate([(2, 1), (1, n)]):
        _knobs(cs, levels, 1)
        fused, pulls = _get(cs, "MOVE_FUSED"), _get(cs, "MOVE_PULL_LAUNCHES")
        run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv_ddt(
            snd[r].dense.data_ptr(), snd[r].bytes, snd[r].doff, rxs[k][r].ptr, rddt, rxs[k][r].cnt, rxs[k][r].displs)))
        torch.cuda.synchronize()
        assert [a - b for a, b in zip(_get(cs, "MOVE_FUSED"), fused)] == [1] * n
        assert [a - b for a, b in zip(_get(cs, "MOVE_PULL_LAUNCHES"), pulls)] == [launches] * n, f"MOVE_ROW_LEVELS {levels}"
    for r in range(n):
        rxs[1][r].want = rxs[0][r].want
        sd._same(rxs[0][r], rxs[1][r], f"receive only, rank {r}")


@pytest.mark.parametrize("case", ["knob_at_1", "three"])
def test_not_published_is_unsupported(gpu, pkg, comms, case):
    """sub16 under MOVE_ROW_LEVELS = 1, and three levels under 2: MI355X_ERR_UNSUPPORTED before the rank meets
    anybody, nothing written, the counters stay, and mi355x_move_send_direct_ok says so too"""
    torch, n = gpu, 3
    cs = comms(n)
    sname = "sub16" if case == "knob_at_1" else "three"
    _knobs(cs, 1 if case == "knob_at_1" else 2, 1)
    snd = [Send(torch, sname, [2] * n, 6000 + q) for q in range(n)]
    rx = [Recv(torch, None, [snd[q].bytes[r] for q in range(n)]) for r in range(n)]
    sddt = snd[0].lay.ddt(pkg)
    assert sddt.row_levels() == (2 if case == "knob_at_1" else 0)
    before = [_get(cs, k) for k in ("MOVE_SEND_DIRECT", "MOVE_FUSED", "MOVE_PULL_LAUNCHES")]
    seen = []

    def rank(r):
        torch.cuda.set_device(0)
        assert not cs[r].move_send_direct_ok(sddt, snd[r].cnt)
        with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):
            cs[r].alltoallv_ddt2(snd[r].ptr, sddt, snd[r].cnt, snd[r].displs, rx[r].ptr, None, rx[r].cnt, rx[r].displs)
        seen.append(r)

    run_ranks(n, rank)
    assert sorted(seen) == list(range(n))
    torch.cuda.synchronize()
    assert [_get(cs, k) for k in ("MOVE_SEND_DIRECT", "MOVE_FUSED", "MOVE_PULL_LAUNCHES")] == before
    for r in range(n):
        assert bool((rx[r].t == POISON).all()) and snd[r].unchanged()
    if case == "knob_at_1":      # the other value of the knob: the same layout is published
        _knobs(cs, 2, 1)
        assert cs[0].move_send_direct_ok(sddt, snd[0].cnt)
    run_alltoallv(torch, pkg, cs, "sub16", None, [[1] * n] * n, min_run=8, what="after the refusals")


def test_truncation_is_refused(gpu, pkg, comms):
    """a receiver one instance short of what a two-level sender sends: MI355X_ERR_TRUNCATE on every rank,
    nothing written, and the next call is exact"""
    torch, n = gpu, 3
    cs = comms(n)
    _knobs(cs, 2, 8)
    snd = [Send(torch, "sub16", [2] * n, 5000 + q) for q in range(n)]
    rx = [Recv(torch, "sub4", [snd[q].bytes[r] for q in range(n)]) for r in range(n)]
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
    run_alltoallv(torch, pkg, cs, "sub16", "sub4", [[1] * n] * n, min_run=8, what="after the refusals")


def test_knobs(gpu, pkg, comms):
    c = comms(2)[0]
    assert pkg.KNOB["MOVE_ROW_LEVELS"] == 49 and pkg.KNOB["MOVE_PULL_LAUNCHES"] == 50
    for v in (1, 2):
        c.set("MOVE_ROW_LEVELS", v)
        assert c.get("MOVE_ROW_LEVELS") == v
    for v in (0, 3, -1):
        with pytest.raises(pkg.MI355XError, match="move_row_levels out of range"):
            c.set("MOVE_ROW_LEVELS", v)
        assert c.get("MOVE_ROW_LEVELS") == 2                   # a rejected value changes nothing
    assert c.get("MOVE_PULL_LAUNCHES") >= 0
    with pytest.raises(pkg.MI355XError):
        c.set("MOVE_PULL_LAUNCHES", 0)                         # read-only
