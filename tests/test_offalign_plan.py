"""The inputs of the multi-process off-alignment run do what test_offalign_ipc_gpu.py claims: from
the tables of offalign_plan.py alone, every branch of the restated address tests is entered by a
full 16-byte piece of a body, the pull-copy table reaches the three copy forms, and the pipelined
table holds the co-aligned, the mixed and the write-through cases.  No GPU."""
from __future__ import annotations

import pytest

import offalign_plan as plan
import opdata

SVC_MAX = 32 << 10   # the service's default LL limit (any limit of a few slices shows the same)
FORMS = {"vec", "word", "byte"}


def test_tables_respect_the_types():
    for op, ty, esz, align, pairs in plan.SLOTS:
        dt = opdata.dtype_of(ty)
        assert (dt.itemsize, dt.alignment) == (esz, align), ty
        assert all(s % align == 0 and r % align == 0 and 0 <= s < 16 and 0 <= r < 16 for s, r in pairs), ty
        assert any(p != (0, 0) for p in pairs) and (0, 0) not in pairs, ty
    for op, ty, esz, align in plan.PIPE_SLOTS:
        dt = opdata.dtype_of(ty)
        assert (dt.itemsize, dt.alignment) == (esz, align), ty
        for layout in plan.pipe_layouts(esz, align):
            assert all(x % align == 0 and 0 <= x < 16 for r in range(9) for x in plan.pipe_shifts(layout, align, r))
    for op, ty in plan.PULL_SLOTS + plan.RS_SLOTS:
        plan.slot(op, ty)


def test_payload_sizes():
    for op, ty, esz, align, pairs in plan.SLOTS:
        sizes = plan.payload_sizes(esz, SVC_MAX)
        assert all(b % esz == 0 and 0 < b <= SVC_MAX for b in sizes) and len(set(sizes)) == 5
        assert sizes[0] == esz and sizes[1] < plan.LL_SLICE < sizes[2] and sizes[4] == SVC_MAX
        assert sizes[3] > plan.SVC_PASS * plan.LL_SLICE
        assert plan.ll_pieces(sizes[3])[-1][1] == esz   # (a 16-byte element is its own whole piece)


@pytest.mark.parametrize("size", [3, 8])
def test_ll_branches_entered_by_body_pieces(size):
    """ll_read16<SYS> by the sbuf shifts and ll_write16<SYS> by the rbuf shifts (in place: the rbuf
    shift for both): each form by a piece with len == 16, and the word and byte forms by a tail too"""
    loads, stores, tails = set(), set(), set()
    for op, ty, esz, align, pairs in plan.SLOTS:
        for i, arr in plan.ll_cases(pairs):
            for rank in range(size):
                s, r = plan.shifts(pairs, i, arr, rank)
                for nbytes in plan.payload_sizes(esz, SVC_MAX):
                    for off, ln in plan.ll_pieces(nbytes):
                        if ln == 16:
                            loads |= {plan.ll_read16_sys(s, ln), plan.ll_read16_sys(r, ln)}
                            stores.add(plan.ll_write16_sys(r, ln))
                        else:
                            tails |= {plan.ll_read16_sys(s, ln), plan.ll_write16_sys(r, ln)}
    assert loads == FORMS and stores == FORMS
    assert tails >= {"word", "byte"}


@pytest.mark.parametrize("size", [3, 8])
def test_rotated_differs_between_ranks(size):
    for op, ty, esz, align, pairs in plan.SLOTS:
        for i in range(len(pairs)):
            assert len({plan.shifts(pairs, i, "rotated", r) for r in range(size)}) == min(size, len(pairs))
            assert {plan.shifts(pairs, i, "same", r) for r in range(size)} == {pairs[i]}


@pytest.mark.parametrize("size", [3, 8])
def test_pull_copy_table_reaches_every_form(size):
    """allgather: block q from rank q's input into rbuf + q * nbytes; bcast: the root's buffer"""
    ag, bc = set(), set()
    for nb in plan.pull_copy_sizes(SVC_MAX):
        for s, d in plan.PULL_COPY_SHIFTS:
            for q in range(size):
                ag.add(plan.svc_copy_seg(s, (d + q * nb) % 16, nb))
                ag.add(plan.svc_copy_seg((d + q * nb) % 16, (d + q * nb) % 16, nb))   # in place: a peer's block
            bc.add(plan.svc_copy_seg(s, d, nb))
    assert ag == FORMS and bc == FORMS


def _pipe_cases(size):
    for op, ty, esz, align in plan.PIPE_SLOTS:
        for layout in plan.pipe_layouts(esz, align):
            sh = [plan.pipe_shifts(layout, align, r) for r in range(size)]
            for inplace in (False, True):
                for wt in (0, 1):
                    for me in range(size):
                        yield ty, layout, plan.pipe_case(size, esz, me, [s for s, _ in sh], [r for _, r in sh], inplace, wt)


@pytest.mark.parametrize("size", [3, 8])
def test_pipe_table(size):
    cases = list(_pipe_cases(size))
    assert any(c["co_fold"] and c["m"] for _, _, c in cases), "co_fold with a shared non-zero misalignment"
    assert any(not c["co_fold"] for _, _, c in cases), "operands that are not co-aligned"
    assert any(c["co_pull"] not in (0, c["all"]) for _, _, c in cases), "some peers' rbufs co-aligned with mine, some not"
    assert any(any(k["wt"] for k in c["chunks"]) and not all(k["wt"] for k in c["chunks"]) for _, _, c in cases), \
        "a write-through chunk and a fenced one in the same call"
    forms = {k["form"] for _, _, c in cases for k in c["chunks"]}
    assert "scalar" in forms and any(f.startswith("head/body") for f in forms) and any(f.startswith("body") for f in forms)
    assert any(f.endswith("tail") for f in forms), forms
    # the head peel from a shared non-zero misalignment: co_fold, m != 0, and a vector body behind the head
    assert any(c["co_fold"] and c["m"] and any(k["form"].startswith("head/body") for k in c["chunks"]) for _, _, c in cases)


@pytest.mark.parametrize("size", [3, 5, 8, 9])
def test_pipe_blocks(size):
    """three chunks per block, the last one short, blocks of unequal length (ring_block's partition)"""
    for op, ty, esz, align in plan.PIPE_SLOTS:
        count, chunk = plan.pipe_count(size, esz), plan.pipe_chunk_elems(esz)
        blocks = [plan.ring_block(count, size, b) for b in range(size)]
        assert blocks[0][0] == 0 and all(blocks[b][0] + blocks[b][1] == blocks[b + 1][0] for b in range(size - 1))
        # (size + 3 elements over the even share: at 3 ranks they divide evenly, elsewhere 3 blocks are longer)
        assert sum(ln for _, ln in blocks) == count and len({ln for _, ln in blocks}) == (1 if size == 3 else 2)
        assert all(2 * chunk < ln < 3 * chunk for _, ln in blocks)
        assert chunk * esz % 16 == 0
    assert plan.pipe_case(size, 4, 0, [0] * size, [0] * size, False, 1)["load_groups"] == (2 if size == 9 else 1)


def test_call_counts_are_positive():
    for size in (3, 5, 8):
        assert plan.ll_reduction_calls(size, SVC_MAX) > 1000 and plan.ll_copy_calls(size, SVC_MAX) == 64
        assert plan.pull_copy_calls(size, SVC_MAX) == 48
    assert plan.pull_calls(SVC_MAX) == (12, 12) and plan.rs_calls() == 32
    assert plan.pipe_calls() == 68 and plan.pipe_two_phase_calls() == 34
