"""The fixtures of tests/large_pyramid_cases.py have teeth (CPU): every case is exact in every mode it is run in, makes the
trips it is for at the table sizes read from the kernels' sources, holds a weight-1 sample on both sides of every cut, and
every emulated wrong pipeline — a trip cut one cell off, a level left out of a later trip, a ragged slot base off by a
level — gives a grad_value that differs from the reference in float32 and after one rounding to bf16."""
import os

import numpy as np
import pytest
import torch

import exact_cases as ec
import large_pyramid_cases as lp
from exact_cases import BF16, F32

RUNS = pytest.mark.parametrize("name,pm,ac", lp.RUNS, ids=lp.RUN_IDS)


def test_table_sizes_are_read_from_the_kernel_sources():
    k = lp.pipeline_constants()
    assert k["kCellLdsInts"] % k["kScanCells"] == 0 and k["kPlaceCellsTwoPerCu"] < k["kCellLdsInts"]
    assert lp.table_sizes() == (k["kCellLdsInts"], k["kPlaceCellsTwoPerCu"])


SORTED_KEYS = ("value_cell_cap", "value_place_cells", "value_place_variant", "value_slices", "value_rounds", "value_win")


def test_the_library_knows_the_sorted_pipelines_counters():
    """every key of `_lib.LAUNCH_INFO_KEYS` is answered by name (0 before the first launch), an unknown one is an error, the
    six counters of the sorted pipeline sit in front of the three grid-form counters, which stay the last three"""
    from msda_triton_amd import _lib
    assert _lib.GRID_FORM_KEYS == ("grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches")
    assert _lib.LAUNCH_INFO_KEYS[-9:-3] == SORTED_KEYS and len(set(_lib.LAUNCH_INFO_KEYS)) == len(_lib.LAUNCH_INFO_KEYS) == 28
    assert _lib.LAUNCH_INFO_KEYS[-11:-9] == ("fwd_trips", "sample_trips")  # (the passes over a unit's samples, in front of those)
    lib = _lib.load()
    for k in _lib.LAUNCH_INFO_KEYS:
        assert int(lib.msda_last_launch_info(k.encode())) >= 0, k
    assert int(lib.msda_last_launch_info(b"value_cell_caps")) < 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msda_hip.h")).read()
    for k in SORTED_KEYS:
        assert f'"{k}"' in header, k


def test_cuts_of_a_hand_made_pyramid():
    # cells 12 + 6 = 18: cstart [0, 12]; count cuts every 5 cells, place cuts every 4 cells of a level
    assert lp.cell_starts([(2, 3), (1, 2)]) == ([0, 12], 18)
    assert lp.cuts([(2, 3), (1, 2)], 5, 4) == ([5, 10, 15], [4, 8, 16])
    assert lp.trips([(2, 3), (1, 2)], 5, 4) == (4, [3, 2])
    assert lp.cuts([(2, 3), (1, 2)], 18, 12) == ([], [])


@pytest.mark.parametrize("name", lp.NAMES)
def test_every_case_makes_the_trips_it_is_for(name):
    levels = lp.levels_of(name)
    cell_cap, place_cells = lp.table_sizes()
    count_trips, place_trips = lp.trips(levels, cell_cap, place_cells)
    print(f"{name}: {lp.cell_starts(levels)[1]} cells, {count_trips} count trips, place trips {place_trips}")
    assert count_trips >= lp.BIG[name][4] >= 2
    big = [(h + 1) * (w + 1) > place_cells for h, w in levels]
    assert any(big) and all(t >= 2 for t, b in zip(place_trips, big) if b)
    B, Q, H, D, _, P = lp.BIG[name][1]
    k = lp.pipeline_constants()
    if name == "big_wide":  # the walk without a fixed slot per thread, one query per place round
        assert len(levels) * P > k["kCellBlock"] and k["kPlaceBlock"] // P == 1
    else:
        assert (sum(P) if isinstance(P, list) else len(levels) * P) <= k["kCellBlock"]
    if name == "big_three":
        assert place_trips == [3, 2]
    if name == "big_u":  # two query slices (sorted_ws_layout)
        import query_mask_cases as qmc
        assert qmc.cell_slices(B, sum(h * w for h, w in levels), H, Q, len(levels) * P) == 2


def test_the_aligned_cut_is_a_level_boundary():
    levels = lp.levels_of("big_aligned")
    count, _ = lp.cuts(levels, *lp.table_sizes())
    assert count == [lp.cell_starts(levels)[0][1]]


@RUNS
def test_precondition_holds(name, pm, ac):
    bud = lp.precondition(name, pm, ac)
    print(f"{name} {pm} {ac}: budget {bud}")
    assert max(bud.values()) <= ec.F32_BITS


@RUNS
def test_a_sample_sits_on_both_sides_of_every_cut(name, pm, ac):
    """... of weight 1, with a grad_out row that is not zero; and a straddled level has samples on both sides of its cut"""
    c = ec.get_case(name)
    d = ec.dense(c)
    levels = lp.levels_of(name)
    cells = lp.sample_cells(c, pm, ac, lp.is_discrete(name))
    heavy = lp.real_mask(c) & (d["attn"] == 1.0) & (d["grad_out"] != 0).any(-1)[:, :, :, None, None]
    targets = lp.planted_targets(name, pm, ac)
    count, place = lp.cuts(levels, *lp.table_sizes())
    assert sorted({t[0] for t in targets}) == sorted(set(count + place)) and len(targets) == 2 * len(set(count + place))
    for cut, side, cell, l, x, y in targets:
        assert (cell < cut) if side == "before" else (cell >= cut)
        assert lp.level_of_cell(levels, cell) == l == lp.level_of_cell(levels, cut - 1 if side == "before" else cut)
        # the nearest cell that can hold a sample: within two cell rows of the cut
        assert abs(cell - (cut - 1 if side == "before" else cut)) <= 2 * (levels[l][1] + 1), (cut, side, cell)
        assert (heavy & (cells == cell)).any(), f"{name} {pm} {ac}: no planted sample in cell {cell} ({side} cut {cut})"
    lvl = np.broadcast_to(np.arange(len(levels)).reshape(1, 1, 1, -1, 1), cells.shape)
    cs, _ = lp.cell_starts(levels)
    real = lp.real_mask(c)
    for cut in count:
        l = lp.level_of_cell(levels, cut)
        if cs[l] != cut:
            here = real & (lvl == l) & (cells >= 0)
            assert (here & (cells < cut)).sum() >= 8 and (here & (cells >= cut)).sum() >= 8, (name, cut)


@RUNS
def test_the_gather_formulation_equals_the_oracle(name, pm, ac):
    ref = lp.checked_reference(name, pm, ac)
    gv = lp.gather_grad_value(ec.get_case(name), pm, ac, None, lp.is_discrete(name))
    assert np.array_equal(gv, ref["grad_value"])


@RUNS
def test_every_wrong_pipeline_differs(name, pm, ac):
    ref = lp.checked_reference(name, pm, ac)
    c = ec.get_case(name)
    mutants = lp.mutants_of(name)
    assert set(lp.MUTANTS[:3]) <= set(mutants)
    if name in ("big_u", "big_c", "big_d", "big_three"):
        assert set(lp.MUTANTS[:5]) <= set(mutants)
    if name == "big_c":
        assert lp.MUTANTS[5] in mutants
    for m in mutants:
        mult = lp.multiplicity(name, pm, ac, m)
        hit = int((lp.real_mask(c) & (mult != 1)).sum())
        gv = torch.from_numpy(lp.gather_grad_value(c, pm, ac, mult, lp.is_discrete(name)))
        off32 = int((gv.to(F32) != ec.expected(ref["grad_value"], F32)).sum())
        off16 = int((gv.to(F32).to(BF16) != ec.expected(ref["grad_value"], BF16)).sum())
        print(f"{name} {pm} {ac} {m}: {hit} samples, {off32} float32 / {off16} bf16 elements of grad_value off")
        assert hit > 0 and off32 > 0 and off16 > 0, (name, pm, ac, m)
