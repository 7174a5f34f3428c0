"""The guarded allocation rig (tests/guarded_alloc.py) on the CPU: the same wrapper with device="cpu", with stand-in
"kernels" that break the buffer contract in the four ways the GPU tests are there to catch.  Each must be reported, with
the tensor and the offset; the well-behaved stand-in passes."""
import pytest
import torch

import guarded_alloc as ga
from guarded_alloc import BAND, FILLS, GuardedAlloc, contract_violations

ROWS, COLS = 6, 8
X = torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) + 1.0


def _launcher(kernel):
    """a stand-in launcher: one output and one scratch table from torch.empty, then the "kernel" """
    def call():
        out = torch.empty((ROWS, COLS), dtype=torch.float32, device="cpu")
        ws = torch.empty(64, dtype=torch.uint8, device="cpu")
        kernel(out, ws)
        return out
    return call


def k_good(out, ws):
    ws.zero_()
    out.copy_(X + ws[0].float())


def k_store_before(out, ws):
    k_good(out, ws)
    out.as_strided((1,), (1,), out.storage_offset() - 1).fill_(0.0)  # one element in front of row 0 (zero bytes: the pattern has none)


def k_store_behind(out, ws):
    k_good(out, ws)
    out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(0.0)  # one element behind the last row


def k_row_unwritten(out, ws):
    ws.zero_()
    out[:ROWS - 1].copy_(X[:ROWS - 1])


def k_reads_scratch_first(out, ws):
    out.copy_(X + ws[3].float())  # a count table that was never initialised
    ws.zero_()


def test_interior_is_aligned_prefilled_and_banded():
    for fill in FILLS:
        with GuardedAlloc(fill, "cpu") as rig:
            t = torch.empty((3, 5), dtype=torch.float64, device="cpu")
            z = torch.empty(0, dtype=torch.uint8, device="cpu")
            h = torch.empty(7, dtype=torch.float16, device=torch.device("cpu"))
            other = torch.empty(4)  # (no device given: not the launchers' form, served by torch)
        assert torch.empty is rig._real  # restored
        assert len(rig.served) == 3 and rig.interiors[0] is t and rig.interiors[1] is z and rig.interiors[2] is h
        assert other.shape == (4,)
        assert rig.allocations == [dict(shape=(3, 5), dtype=torch.float64, bytes=120), dict(shape=(0,), dtype=torch.uint8, bytes=0),
                                   dict(shape=(7,), dtype=torch.float16, bytes=14)]
        for a in rig.served:
            assert a.interior.data_ptr() % 256 == 0 and a.interior.is_contiguous()
            assert a.start >= BAND and a.backing.numel() - a.start - a.nbytes >= BAND
            assert bool((ga.as_bytes(a.interior) == fill).all())
            assert bool((a.backing[:a.start] != 0).all()) and bool((a.backing[a.start + a.nbytes:] != 0).all())
        assert all(r["front"] is None and r["back"] is None for r in rig.report()) and not rig.band_violations()
    with GuardedAlloc(0xFF, "cpu"):
        for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            assert bool(torch.isnan(torch.empty(9, dtype=dt, device="cpu")).all())  # 0xFF bytes: NaN in every float type


def test_well_behaved_stand_in_passes():
    bad, rigs, results = contract_violations(_launcher(k_good), 2, "cpu")
    assert not bad, bad
    assert [len(r.served) for r in rigs] == [2, 2]
    for res in results:
        assert torch.equal(res[0], X)


@pytest.mark.parametrize("kernel,side,offset", [(k_store_before, "front", -1), (k_store_behind, "back", 0)],
                         ids=["one_element_before", "one_element_behind"])
def test_a_store_outside_the_interior_is_reported_with_its_offset(kernel, side, offset):
    """(run under the rig only: without it the stand-in would write into the allocator's own memory)"""
    for fill in FILLS:
        with GuardedAlloc(fill, "cpu") as rig:
            out = _launcher(kernel)()
        assert torch.equal(out, X)  # the result itself looks right: only the band tells
        rep = rig.report()
        other = "back" if side == "front" else "front"
        # the four bytes of the stray float: the byte nearest the interior is reported
        assert rep[0][side] == offset and rep[0][other] is None, rep[0]
        assert rep[1]["front"] is None and rep[1]["back"] is None
        v = rig.band_violations()
        assert len(v) == 1 and "allocation 0" in v[0] and side in v[0] and f"offset {offset}" in v[0], v
    with GuardedAlloc(0x5A, "cpu") as rig:  # the far end of either band is still seen
        out = torch.empty(4, dtype=torch.uint8, device="cpu")
        out.as_strided((1,), (1,), out.storage_offset() - BAND).fill_(0)
        out.as_strided((1,), (1,), out.storage_offset() + 4 + BAND - 1).fill_(0)
    assert rig.report()[0]["front"] == -BAND and rig.report()[0]["back"] == BAND - 1


def test_an_unwritten_row_is_reported():
    bad, _, results = contract_violations(_launcher(k_row_unwritten), 2, "cpu", names=["out"])
    first = (ROWS - 1) * COLS
    assert any("still hold the pre-fill" in v and f"(element {first})" in v and "out" in v for v in bad), bad
    assert any("pre-fill 0xFF" in v and "not finite" in v and f"element {first}" in v for v in bad), bad
    assert bool(torch.isnan(results[1][0][ROWS - 1]).all())  # the 0xFF run: the row's NaN survived


def test_a_scratch_table_read_before_it_is_written_is_reported():
    bad, _, results = contract_violations(_launcher(k_reads_scratch_first), 2, "cpu", names=["out"])
    assert any("differs from the run without the rig" in v for v in bad), bad
    assert not ga.bits_equal(results[1][0], results[2][0])  # the result follows the pre-fill
    assert not any("band" in v for v in bad)


def test_a_bypassed_rig_is_a_failure():
    def call():  # allocates without the launchers' form: nothing is served
        out = torch.zeros(ROWS, COLS)
        out.copy_(X)
        return out
    bad, _, _ = contract_violations(call, 1, "cpu")
    assert any("served 0 allocations, the launcher makes 1" in v for v in bad), bad
    bad, _, _ = contract_violations(_launcher(k_good), 3, "cpu")
    assert any("served 2 allocations, the launcher makes 3" in v for v in bad), bad


def test_unmodelled_arguments_are_refused_not_passed_through():
    with GuardedAlloc(0xFF, "cpu"):
        with pytest.raises(AssertionError):
            torch.empty(3, device="cpu", pin_memory=False)
