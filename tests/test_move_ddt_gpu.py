"""gather(v), scatter(v), allgatherv and alltoall(v) pulling straight into a derived receive datatype
(mi355x_*_ddt, coll_move.cpp; the multi-segment row unpack of ddt_kernels.hip) on loopback
communicators, one thread per rank.

Every result is compared byte for byte with two references: a numpy placement computed from the
layout as written out in tests/move_ddt_model.py, and the unfused sequence the calls replace -- the
plain engine call into dense bytes, then Ddt.unpack per piece.  Receive buffers start as poison with
guard bytes either side: the layout's gaps and the guards must keep it.  Layouts are the smallest
that reach each branch: slot widths 4, 16, 8 (pieces interleaved) and 1 of the one-launch row kernel,
a three-run layout (piece by piece), a gap-free one (the plain call); ragged counts with an empty
piece, a one-instance piece beside one of 5000 instances and a sender that stops inside a run; a
receive base 4 bytes off 16-byte alignment; the MOVE_FUSED counter; MPI_IN_PLACE refused.
"""
from __future__ import annotations

import numpy as np
import pytest

import move_ddt_model as mdl
from test_coll_gpu import run_ranks

pytestmark = pytest.mark.gpu

G, POISON = mdl.GUARD, mdl.POISON


@pytest.fixture(scope="module")
def comms(gpu, pkg):
    made = {}

    def get(n):
        if n not in made:
            made[n] = pkg.Comm.loopback(n, 0)
        return made[n]

    yield get
    for cs in made.values():
        for c in cs:
            c.destroy()


def _layout(name):
    """the layout and, for receiver-side counts cnt[q], the byte displacement of every piece"""
    if name == "col8":
        rows = 50

        def build(cnt):
            ncols = sum(cnt) + 1                     # one spare column: a gap that keeps the poison
            lay = mdl.column(rows, ncols)
            first = np.concatenate([[0], np.cumsum(cnt[:-1])])
            return lay, [int(c) * 8 for c in first], rows * ncols * 8
        return build
    lay = {"vec37": mdl.vec37, "vec9": mdl.vec9, "odd3": mdl.odd3, "idx3": mdl.idx3, "contig": mdl.contiguous}[name]()

    def build(cnt):
        displs, at = [], 0
        for c in cnt:
            displs.append(at)
            at += (lay.span(c) + 15) // 16 * 16 + 32   # pieces 16-byte aligned, 32 poison bytes between
        return lay, displs, at
    return build


class Recv:
    """one rank's receive side: a poisoned device buffer with guards, `off` bytes off 16-byte alignment"""

    def __init__(self, torch, total, off=0):
        self.t = torch.full((total + 2 * G + 16,), POISON, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        self.lo = G + off
        self.ptr = self.t.data_ptr() + self.lo
        self.want = np.full(total + 2 * G + 16, POISON, dtype=np.uint8)

    def got(self):
        return self.t.cpu().numpy()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unfused(torch, ddt, rx, dense, offs, cnt, displs, sent):
    """the parent's receive: the dense bytes of every piece unpacked with one launch each"""
    for q in range(len(cnt)):
        if sent[q]:
            ddt.unpack(cnt[q], rx.ptr + displs[q], 0, dense.data_ptr() + offs[q], sent[q])
    torch.cuda.synchronize()


def _dense_offsets(caps):
    return [int(v) for v in np.concatenate([[0], np.cumsum(caps[:-1])])]


def _check(rx_fused, rx_plain, what):
    want = rx_fused.want
    got = rx_fused.got()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: fused differs from the numpy model at byte {bad[0] - rx_fused.lo} (+{bad.size - 1} more)"
    ref = rx_plain.got()
    bad = np.nonzero(ref != want)[0]
    assert bad.size == 0, f"{what}: the unfused sequence differs from the numpy model at byte {bad[0] - rx_plain.lo}"
    assert np.array_equal(got, ref), what


def _fused_delta(cs, before, expect, what):
    for r, c in enumerate(cs):
        assert c.get("MOVE_FUSED") - before[r] == expect[r], f"{what}: MOVE_FUSED on rank {r}"


def run_alltoallv(torch, pkg, cs, build, counts, sent, off=0, what=""):
    """counts[r][q]: instances receiver r holds for sender q; sent[q][r]: bytes q sends to r"""
    n = len(cs)
    sides = [build(counts[r]) for r in range(n)]
    ddts = [sides[r][0].ddt(pkg) for r in range(n)]
    sdis = [[int(v) + 16 * r for r, v in enumerate(np.concatenate([[0], np.cumsum(sent[q][:-1])]))] for q in range(n)]
    data = [[mdl.payload(1000 * q + r, sent[q][r]) for r in range(n)] for q in range(n)]
    sbuf = []
    for q in range(n):
        h = np.full(sdis[q][-1] + sent[q][-1] + 16, 0x5A, dtype=np.uint8)
        for r in range(n):
            h[sdis[q][r]:sdis[q][r] + sent[q][r]] = data[q][r]
        sbuf.append(_dev(torch, h))
    rxf = [Recv(torch, sides[r][2], off) for r in range(n)]
    rxp = [Recv(torch, sides[r][2], off) for r in range(n)]
    caps = [[counts[r][q] * sides[r][0].size for q in range(n)] for r in range(n)]
    dense = [torch.full((sum(caps[r]) + 16,), 0x77, dtype=torch.uint8, device="cuda") for r in range(n)]
    for r in range(n):
        for q in range(n):
            mdl.place(rxf[r].want, rxf[r].lo, sides[r][0], sides[r][1][q], data[q][r])
    torch.cuda.synchronize()
    before = [c.get("MOVE_FUSED") for c in cs]
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv_ddt(
        sbuf[r].data_ptr(), sent[r], sdis[r], rxf[r].ptr, ddts[r], counts[r], sides[r][1])))
    gap_free = sides[0][0].name == "contig"
    _fused_delta(cs, before, [0 if gap_free or not any(sent[q][r] for q in range(n)) else 1 for r in range(n)], what)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].alltoallv(
        sbuf[r].data_ptr(), sent[r], sdis[r], dense[r].data_ptr(), caps[r], _dense_offsets(caps[r]))))
    for r in range(n):
        _unfused(torch, ddts[r], rxp[r], dense[r], _dense_offsets(caps[r]), counts[r], sides[r][1],
                 [sent[q][r] for q in range(n)])
        _check(rxf[r], rxp[r], f"{what} alltoallv rank {r}")


def run_gatherv(torch, pkg, cs, build, cnt, sent, root, off=0, what=""):
    """the root holds cnt[q] instances for rank q, which sends sent[q] bytes"""
    n = len(cs)
    lay, displs, total = build(cnt)
    ddt = lay.ddt(pkg)
    data = [mdl.payload(2000 + q, sent[q]) for q in range(n)]
    sbuf = [_dev(torch, np.concatenate([data[q], np.zeros(16, np.uint8)])) for q in range(n)]
    rxf, rxp = Recv(torch, total, off), Recv(torch, total, off)
    caps = [c * lay.size for c in cnt]
    dense = torch.full((sum(caps) + 16,), 0x77, dtype=torch.uint8, device="cuda")
    for q in range(n):
        mdl.place(rxf.want, rxf.lo, lay, displs[q], data[q])
    torch.cuda.synchronize()
    before = [c.get("MOVE_FUSED") for c in cs]
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv_ddt(
        sbuf[r].data_ptr(), sent[r], rxf.ptr if r == root else None, ddt, cnt if r == root else None,
        displs if r == root else None, root)))
    _fused_delta(cs, before, [1 if r == root and lay.name != "contig" and any(sent) else 0 for r in range(n)], what)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].gatherv(
        sbuf[r].data_ptr(), sent[r], dense.data_ptr() if r == root else None, caps if r == root else None,
        _dense_offsets(caps) if r == root else None, root)))
    _unfused(torch, ddt, rxp, dense, _dense_offsets(caps), cnt, displs, sent)
    _check(rxf, rxp, f"{what} gatherv root {root}")


def run_scatterv(torch, pkg, cs, build, cnt, sent, root, off=0, what=""):
    """rank r holds cnt[r] instances and the root sends it sent[r] bytes"""
    n = len(cs)
    data = [mdl.payload(3000 + r, sent[r]) for r in range(n)]
    sdis = [int(v) + 16 * r for r, v in enumerate(np.concatenate([[0], np.cumsum(sent[:-1])]))]
    h = np.full(sdis[-1] + sent[-1] + 16, 0x5A, dtype=np.uint8)
    for r in range(n):
        h[sdis[r]:sdis[r] + sent[r]] = data[r]
    sbuf = _dev(torch, h)
    sides = [build([cnt[r]]) for r in range(n)]
    ddts = [sides[r][0].ddt(pkg) for r in range(n)]
    rxf = [Recv(torch, sides[r][2], off) for r in range(n)]
    rxp = [Recv(torch, sides[r][2], off) for r in range(n)]
    caps = [cnt[r] * sides[r][0].size for r in range(n)]
    dense = [torch.full((caps[r] + 16,), 0x77, dtype=torch.uint8, device="cuda") for r in range(n)]
    for r in range(n):
        mdl.place(rxf[r].want, rxf[r].lo, sides[r][0], 0, data[r])
    torch.cuda.synchronize()
    before = [c.get("MOVE_FUSED") for c in cs]
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv_ddt(
        sbuf.data_ptr() if r == root else None, sent if r == root else None, sdis if r == root else None,
        rxf[r].ptr, ddts[r], cnt[r], root)))
    _fused_delta(cs, before, [1 if sides[r][0].name != "contig" and sent[r] else 0 for r in range(n)], what)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].scatterv(
        sbuf.data_ptr() if r == root else None, sent if r == root else None, sdis if r == root else None,
        dense[r].data_ptr(), caps[r], root)))
    for r in range(n):
        _unfused(torch, ddts[r], rxp[r], dense[r], [0], [cnt[r]], [0], [sent[r]])
        _check(rxf[r], rxp[r], f"{what} scatterv rank {r}")


def run_allgatherv(torch, pkg, cs, build, cnt, off=0, what=""):
    """every rank holds cnt[q] instances for rank q, which sends exactly that"""
    n = len(cs)
    lay, displs, total = build(cnt)
    ddt = lay.ddt(pkg)
    caps = [c * lay.size for c in cnt]
    data = [mdl.payload(4000 + q, caps[q]) for q in range(n)]
    sbuf = [_dev(torch, np.concatenate([data[q], np.zeros(16, np.uint8)])) for q in range(n)]
    rxf = [Recv(torch, total, off) for _ in range(n)]
    rxp = [Recv(torch, total, off) for _ in range(n)]
    dense = [torch.full((sum(caps) + 16,), 0x77, dtype=torch.uint8, device="cuda") for _ in range(n)]
    for r in range(n):
        for q in range(n):
            mdl.place(rxf[r].want, rxf[r].lo, lay, displs[q], data[q])
    torch.cuda.synchronize()
    before = [c.get("MOVE_FUSED") for c in cs]
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv_ddt(
        sbuf[r].data_ptr(), caps[r], rxf[r].ptr, ddt, cnt, displs)))
    _fused_delta(cs, before, [1 if lay.name != "contig" and any(caps) else 0] * n, what)
    run_ranks(n, lambda r: (torch.cuda.set_device(0), cs[r].allgatherv(
        sbuf[r].data_ptr(), caps[r], dense[r].data_ptr(), caps, _dense_offsets(caps))))
    for r in range(n):
        _unfused(torch, ddt, rxp[r], dense[r], _dense_offsets(caps), cnt, displs, caps)
        _check(rxf[r], rxp[r], f"{what} allgatherv rank {r}")


def _counts(n, r):
    return [1 + (3 * q + r) % 5 for q in range(n)]     # 1..5 instances: vec9's 5 x 144 slots is no whole block


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("name", ["vec37", "vec9", "col8", "odd3", "idx3", "contig"])
def test_four_calls(gpu, pkg, comms, n, name):
    """every call into every layout, whole pieces; the gap-free layout is the plain call (MOVE_FUSED stays)"""
    torch, cs, build = gpu, comms(n), _layout(name)
    what = f"{name} n={n}"
    counts = [_counts(n, r) for r in range(n)]
    size = build(counts[0])[0].size
    run_alltoallv(torch, pkg, cs, build, counts, [[counts[r][q] * size for r in range(n)] for q in range(n)], what=what)
    for root in sorted({0, n - 1}):
        run_gatherv(torch, pkg, cs, build, counts[root], [c * size for c in counts[root]], root, what=what)
        run_scatterv(torch, pkg, cs, build, counts[root], [c * size for c in counts[root]], root, what=what)
    run_allgatherv(torch, pkg, cs, build, counts[1], what=what)


def _ragged(n, r, lay_run, size):
    """piece q of receiver r: one instance, 5000 instances, none, or three of which the sender fills one
    instance, one run and 5 bytes more -- the window ends inside a run"""
    cnt, sent = [], []
    for q in range(n):
        kind = ("one", "big", "zero", "part")[(q + 2 * r) % 4]
        c = {"one": 1, "big": 5000, "zero": 0, "part": 3}[kind]
        cnt.append(c)
        sent.append(size + lay_run + 5 if kind == "part" else c * size)
    return cnt, sent


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("name", ["vec37", "col8"])
def test_ragged(gpu, pkg, comms, n, name):
    """an empty piece, a piece smaller than a block beside one spanning many, a sender that stops inside a
    run: the bytes beyond its window stay poison"""
    torch, cs, build = gpu, comms(n), _layout(name)
    lay = build([1])[0]
    assert 5 < lay.run, "the short window ends inside a run"
    rag = [_ragged(n, r, lay.run, lay.size) for r in range(n)]
    counts = [rag[r][0] for r in range(n)]
    sent = [[rag[r][1][q] for r in range(n)] for q in range(n)]
    what = f"ragged {name} n={n}"
    run_alltoallv(torch, pkg, cs, build, counts, sent, what=what)
    for root in (0, 1):
        run_gatherv(torch, pkg, cs, build, rag[root][0], rag[root][1], root, what=what)
    cnt = [rag[r][0][(r + 1) % n] for r in range(n)]
    run_scatterv(torch, pkg, cs, build, cnt, [rag[r][1][(r + 1) % n] for r in range(n)], n - 1, what=what)
    run_allgatherv(torch, pkg, cs, build, [min(c, 700) for c in rag[0][0]], what=what)


@pytest.mark.parametrize("name", ["vec9", "col8", "idx3"])
def test_base_off_alignment(gpu, pkg, comms, name):
    """the receive base 4 bytes past a 16-byte boundary: the whole launch drops to 4-byte slots"""
    n = 3
    torch, cs, build = gpu, comms(n), _layout(name)
    counts = [_counts(n, r) for r in range(n)]
    size = build(counts[0])[0].size
    run_alltoallv(torch, pkg, cs, build, counts, [[counts[r][q] * size for r in range(n)] for q in range(n)], off=4,
                  what=f"{name} base+4")
    run_gatherv(torch, pkg, cs, build, counts[2], [c * size for c in counts[2]], 2, off=4, what=f"{name} base+4")


@pytest.mark.parametrize("n", [2, 8])
def test_inplace_is_unsupported(gpu, pkg, comms, n):
    """MPI_IN_PLACE with a layout: MI355X_ERR_UNSUPPORTED before the rank meets anybody (every rank makes
    the call, the gatherv root makes it alone), nothing written; the communicator serves the next call"""
    torch, cs = gpu, comms(n)
    lay = mdl.vec37()
    ddt = lay.ddt(pkg)
    cnt = [2] * n
    displs = [q * 2048 for q in range(n)]
    bufs = [torch.full((2048 * n,), POISON, dtype=torch.uint8, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    before = [c.get("MOVE_FUSED") for c in cs]
    seen = []

    def rank(r):
        torch.cuda.set_device(0)
        for call in (lambda: cs[r].allgatherv_ddt(None, 0, bufs[r].data_ptr(), ddt, cnt, displs),
                     lambda: cs[r].alltoallv_ddt(None, None, None, bufs[r].data_ptr(), ddt, cnt, displs)):
            with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):
                call()
            seen.append(r)

    run_ranks(n, rank)
    assert sorted(seen) == sorted(list(range(n)) * 2)
    with pytest.raises(pkg.MI355XError, match="MI355X_ERR_UNSUPPORTED"):
        cs[n - 1].gatherv_ddt(None, 0, bufs[n - 1].data_ptr(), ddt, cnt, displs, n - 1)
    torch.cuda.synchronize()
    for r in range(n):
        assert bool((bufs[r] == POISON).all()), f"rank {r}'s buffer was written"
        assert cs[r].get("MOVE_FUSED") == before[r]
    build = _layout("vec37")
    run_allgatherv(torch, pkg, cs, build, [1] * n, what="after the refusals")


def test_knob_is_read_only(gpu, pkg, comms):
    c = comms(2)[0]
    assert pkg.KNOB["MOVE_FUSED"] == 46
    with pytest.raises(pkg.MI355XError):
        c.set("MOVE_FUSED", 0)
