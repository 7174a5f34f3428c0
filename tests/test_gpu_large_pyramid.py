"""grad_value on pyramids LARGER than the sorted pipeline's LDS tables, with NO tolerance: the fixtures of
tests/large_pyramid_cases.py (exact inputs; a weight-1 sample on both sides of every trip cut;
tests/test_large_pyramid_cases.py shows that a pipeline which cuts a trip one cell off, leaves a level out of a later trip
or re-bases a ragged trip's slots by the wrong level gives another grad_value) through every instantiation of the count,
place, scan and finish passes: the storages, per-level counts, discrete sampling, the value-mask and query-mask kernargs,
the walk without a fixed slot per thread, both place passes, rounds of queries, passes over the batch and records in the
caller's gradient buffers.  Every comparison of the plain operator is an EQUALITY of out, grad_value, grad_loc and
grad_attn with the fp64 reference rounded once; only the fused families, whose softmax is not exact, carry the project's
FWD_TOL / BWD_TOL.  Every test reads the trips it reached off `msda_last_launch_info` ("value_cell_cap",
"value_place_cells") and asserts them, and that the table sizes are the ones the fixtures' samples were planted for.
Run with ``-m gpu``."""
import functools

import numpy as np
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
import large_pyramid_cases as lp
import query_mask_cases as qmc
from exact_cases import MODES
from test_gpu_exact_numerics import DEV, MODE_IDS, STORAGE, assert_exact, launch_info, options, run

pytestmark = pytest.mark.gpu

TWO_MODES = [("zeros", False), ("border", True)]
TWO_IDS = ["zeros_0", "border_1"]


def assert_trips(name, info, passes=1, variant=None):
    """The launch took the sorted pipeline with the tables the fixture was planted for, and made the trips it is for."""
    levels = lp.levels_of(name)
    cell_cap, place_cells = lp.table_sizes()
    _, total = lp.cell_starts(levels)
    assert info["value_path"] == 2 and info["value_passes"] == passes, info
    assert info["value_cell_cap"] == cell_cap, (info, cell_cap)
    count_trips = -(-total // info["value_cell_cap"])
    if variant is not None:
        assert info["value_place_variant"] == variant, info
    if info["value_place_variant"] == 0:  # the plane-major place pass: the count pass's table and trips
        assert info["value_place_cells"] == 0, info
        place_trips = [count_trips]
    else:
        assert info["value_place_cells"] == place_cells, (info, place_cells)
        place_trips = [-(-(h + 1) * (w + 1) // info["value_place_cells"]) for h, w in levels]
    print(f"{name}: {total} cells, count trips {count_trips}, place trips {place_trips}, cell_cap {info['value_cell_cap']}, "
          f"place_cells {info['value_place_cells']}, place variant {info['value_place_variant']}, slices {info['value_slices']}, "
          f"rounds {info['value_rounds']}, win {info['value_win']}")
    assert count_trips >= lp.BIG[name][4] and max(place_trips) >= (3 if name == "big_three" else 2), (count_trips, place_trips)
    assert info["value_slices"] >= 1 and info["value_rounds"] >= 1 and info["value_win"] >= 1, info
    return info


def check(name, pm, ac, storage, passes=1, variant=None, **opts):
    vdt, cdt = STORAGE[storage]
    ref = lp.checked_reference(name, pm, ac)
    opts.setdefault("value_path", 2)
    with options(**opts):
        got = run(ec.get_case(name), pm, ac, vdt, cdt)
        info = launch_info()
    assert_exact(got, ref, f"{name} {pm} {int(ac)} {storage} {opts}")
    return assert_trips(name, info, passes, variant)


# ----------------------------------------------------------------------------------------- the route by itself
def test_auto_route_takes_the_sorted_pipeline():
    info = check("big_u", "zeros", False, "f32", value_path=0)
    assert info["value_slices"] == 2, info  # (two query slices: sorted_ws_layout)


# ----------------------------------------------------------------------------------------- storages
@pytest.mark.parametrize("storage", ["f32", "f64", "bf16", "f32_vbf16"])
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
def test_storages_are_exact(pm, ac, storage):
    check("big_u", pm, ac, storage)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("pm,ac", TWO_MODES, ids=TWO_IDS)
@pytest.mark.parametrize("name", ["big_three", "big_aligned"])
def test_three_trips_and_the_aligned_cut_are_exact(name, pm, ac, storage):
    check(name, pm, ac, storage)


# ----------------------------------------------------------------------------------------- both place passes
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("place_path,variant", [(0, 1), (3, 2), (1, 0)], ids=["level_major_1024", "level_major_256", "plane_major"])
def test_place_passes_are_exact(place_path, variant, storage):
    """(the plane-major pass makes the two count-sized trips itself; its record order is not reproducible — strict=0 — but
    the sums are exact in any order)"""
    for pm, ac in MODES:
        check("big_u", pm, ac, storage, variant=variant, place_path=place_path, strict=0)


# ----------------------------------------------------------------------------------------- the walk without a fixed slot
def test_more_slots_than_threads_is_exact():
    k = lp.pipeline_constants()
    L, P = len(lp.levels_of("big_wide")), lp.BIG["big_wide"][1][5]
    assert L * P > k["kCellBlock"]
    for pm, ac in MODES:
        check("big_wide", pm, ac, "f32")


# ----------------------------------------------------------------------------------------- rounds, passes, records
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_rounds_of_queries_are_exact(storage):
    for pm, ac in MODES:
        info = check("big_u", pm, ac, storage, q_round=500)
        assert info["value_rounds"] == 3, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_passes_over_the_batch_are_exact(storage):
    for pm, ac in MODES:
        check("big_u", pm, ac, storage, passes=2, ws_passes=2)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("rig", [0, 1], ids=["records_in_workspace", "records_in_grads"])
def test_records_in_the_callers_gradient_buffers_are_exact(rig, storage):
    for pm, ac in MODES:
        check("big_u", pm, ac, storage, records_in_grads=rig)


# ----------------------------------------------------------------------------------------- per-level point counts
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
def test_points_per_level_is_exact(pm, ac, storage):
    check("big_c", pm, ac, storage)


# ----------------------------------------------------------------------------------------- discrete sampling
@pytest.mark.parametrize("storage", ["f32", "f64", "bf16"])
def test_discrete_sampling_is_exact(storage):
    vdt, cdt = STORAGE[storage]
    ref = lp.checked_reference("big_d")  # (test_discrete_sampling.ref_discrete, cached by exact_cases.reference)
    with options(value_path=2):
        got = run(ec.get_case("big_d"), "border", False, vdt, cdt, discrete=True)
        info = launch_info()
    assert_exact(got, ref, f"big_d {storage}")
    assert info["fwd_variant"] == 3 and info["sample_variant"] == 2, info
    assert_trips("big_d", info)


# ----------------------------------------------------------------------------------------- the value mask
@functools.lru_cache(maxsize=None)
def value_mask():
    from test_gpu_value_mask import make_mask
    B, levels = lp.BIG["big_u"][1][0], lp.levels_of("big_u")
    m = make_mask("bernoulli", B, levels, seed=11)
    assert 0 < int(m.sum()) < m.numel()
    return m


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_value_mask_on_a_poisoned_pyramid_is_exact(storage):
    """NaN in every padding pixel; the masked finish kernel over the plane's 40 200 pixels"""
    vdt, cdt = STORAGE[storage]
    m = value_mask()
    for pm, ac in MODES:
        lp.precondition("big_u", pm, ac)
        ref = ec.masked_reference("big_u", pm, ac, m.numpy())
        with options(value_path=2):
            got = run(ec.get_case("big_u"), pm, ac, vdt, cdt, mask=m)
            info = launch_info()
        assert_exact(got, ref, f"big_u {pm} {int(ac)} {storage} value-masked")
        assert_trips("big_u", info)


# ----------------------------------------------------------------------------------------- the query mask
@functools.lru_cache(maxsize=None)
def query_masked_reference(kind, pm, ac):
    """-> (mask [B, Q] bool on the host, the oracle on the sanitised inputs): exact whenever the unmasked case is (every sum
    runs over a subset of its terms) — budget and float32 == float64 asserted again by query_mask_cases.exact_reference"""
    lp.precondition("big_u", pm, ac)
    qm = qmc.exact_query_mask("big_u", kind)
    _, ref = qmc.exact_reference("big_u", pm, ac, qm.numpy())
    return qm, ref


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["bernoulli", "tail", "slice_edges"])
def test_query_mask_is_exact(kind, storage):
    from msda_triton_amd import multiscale_deformable_attention
    from test_gpu_module_masks import nothing_composed
    vdt, cdt = STORAGE[storage]
    c = ec.get_case("big_u")
    for pm, ac in MODES:
        qm, ref = query_masked_reference(kind, pm, ac)
        v, l, a, go = (torch.from_numpy(np.array(c[k])).to(DEV, dt) for k, dt in
                       (("value", vdt), ("loc", cdt), ("attn", cdt), ("grad_out", cdt)))
        v, l, a = (t.requires_grad_(True) for t in (v, l, a))
        with options(value_path=2), nothing_composed():
            out = multiscale_deformable_attention(v, torch.from_numpy(np.array(c["shapes"])).to(DEV), l, a, pm, ac,
                                                  query_mask=qm.to(DEV))
            out.backward(go)
            torch.cuda.synchronize()
            info = launch_info()
        got = dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_loc=l.grad.cpu(), grad_attn=a.grad.cpu())
        for k in ("out", "grad_loc", "grad_attn"):  # masked rows are zeros
            assert not bool(got[k][~qm].any()), (kind, pm, ac, k)
        # (the oracle's `out` of a sanitised query is zero too: its weights are)
        assert_exact(got, ref, f"big_u {pm} {int(ac)} {storage} query mask {kind}")
        assert_trips("big_u", info)


# ----------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("name", ["big_u", "big_c"])
def test_grad_value_is_reproducible_under_strict(name):
    """two calls under another block -> plane mapping (xcd_map 1 and 0) return bit-identical results: the level-major place
    pass's record order does not depend on which workgroup runs first"""
    ref = lp.checked_reference(name, "zeros", False)
    res = []
    for xcd_map in (1, 0):
        with options(value_path=2, strict=1, xcd_map=xcd_map):
            res.append(run(ec.get_case(name), "zeros", False, torch.float32, torch.float32))
            info = launch_info()
        assert_trips(name, info)
        assert info["value_place_variant"] in (1, 2), info
        assert_exact(res[-1], ref, f"{name} strict xcd_map={xcd_map}")
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


# ----------------------------------------------------------------------------------------- the fused families
from msda_triton_amd import _ext, _lib  # noqa: E402
from test_gpu_parity import BWD_TOL, FWD_TOL  # noqa: E402

FUSED_D = 8


def _draw(family, B, Q, H, levels, per, ref_dim, seed):
    """random inputs as head_dim_cases._fused_draw makes them, on a large pyramid (float32, host)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = len(levels)
    ragged = family in ("ragged", "hfbox")
    value = torch.randn(B, sum(h * w for h, w in levels), H, FUSED_D, generator=g)
    proj = torch.randn((B, Q, H, sum(per), 3) if ragged else (B, Q, H, L, per[0], 3), generator=g) * 1.5
    rshape = {"ragged": (B, Q, ref_dim), "hfbox": (B, Q, 1, 4)}.get(family, (B, Q, L, ref_dim))
    ref = torch.rand(rshape, generator=g)
    gout = torch.rand(B, Q, H, FUSED_D, generator=g)
    mask = (torch.rand(B, value.shape[1], generator=g) < 0.5) if family == "levelref_masked" else None
    return dict(value=value, shapes=torch.tensor(levels), proj=proj, ref=ref, gout=gout, counts=list(per) if ragged else None,
                mask=mask, family=family, seed=seed)


def _assert_one_pass(S):
    limit = int(_lib.load().msda_fused_lp_limit(FUSED_D, 4))
    ext = _ext.load()
    assert S <= limit and (ext is None or int(ext.fused_lp_limit(FUSED_D, 4)) == limit), (S, limit)  # no composition


def _assert_fused_close(got, inp, qm, pm, ac, what):
    """against head_dim_cases.fused_reference on the sanitised inputs at FWD_TOL / BWD_TOL; offsets within 1e-4 of a grid
    kink are left out (at most KINK_CAP of them), and a query's reference-point gradient — the sum over its samples, a
    kink's jump included — is compared when none of its samples sits there (tests/test_gpu_hostile_inputs.py)"""
    pr, rf, go = qmc.sanitised_fused(inp["proj"], inp["ref"], inp["gout"], qm) if qm is not None else (inp["proj"], inp["ref"], inp["gout"])
    san = dict(inp, proj=pr, ref=rf, gout=go)
    want = hd.fused_reference(san, pm, ac)
    if qm is not None:  # the kernels store zeros for a masked query; the reference's `out` row there is the mean of its samples
        want = (torch.where(qm[:, :, None, None], want[0], torch.zeros_like(want[0])),) + tuple(want[1:])
        for i in (0, 2, 3):
            assert not bool(got[i][~qm].any()), (what, i)
    kink = torch.from_numpy(hd.fused_kinks(san, ac))
    assert float(kink.float().mean()) <= hd.KINK_CAP
    keep_q = ~kink.reshape(kink.shape[0], kink.shape[1], -1).any(-1)
    assert float(keep_q.float().mean()) > 0.5
    got, want = [t.clone() for t in got], [t.clone() for t in want]
    for t in (got, want):
        t[2][..., :2] = torch.where(kink, torch.zeros_like(t[2][..., :2]), t[2][..., :2])
        t[3] = torch.where(keep_q.reshape(keep_q.shape + (1,) * (t[3].dim() - 2)), t[3], torch.zeros_like(t[3]))
    tols = [FWD_TOL[torch.float32]] + [BWD_TOL[torch.float32]] * 3
    for nm, g, w, t in zip(("out", "grad_value", "grad_proj", "grad_ref"), got, want, tols):
        print(f"{what} {nm}: largest difference {float((g.double() - w).abs().max()):.3e}")
        torch.testing.assert_close(g, w.to(torch.float32), msg=lambda m: f"{what} {nm}: {m}", **t)


def test_fused_levelref_with_both_masks():
    """the Hugging Face encoder's call: per-level reference points, value mask and query mask — the MaskedParams count and
    place passes over two trips"""
    from msda_triton_amd.functional import KernelTimer, fused_hf_module_core
    from test_gpu_module_masks import nothing_composed
    B, Q, H, _, levels, P = lp.BIG["big_u"][1]
    _assert_one_pass(len(levels) * P)
    inp = _draw("levelref_masked", B, Q, H, levels, [P] * len(levels), 2, 101)
    qm = qmc.make_query_mask("tail", B, Q, 3)
    for pm, ac in TWO_MODES:
        v = torch.where(inp["mask"][:, :, None, None], inp["value"], torch.full_like(inp["value"], float("nan")))
        v, pr, rf = (t.to(DEV).requires_grad_(True) for t in (v, inp["proj"], inp["ref"]))
        with options(value_path=2), nothing_composed(), KernelTimer() as kt:
            out = fused_hf_module_core(v, inp["shapes"].to(DEV), pr, rf, pm, ac, value_mask=inp["mask"].to(DEV), query_mask=qm.to(DEV))
            out.backward(inp["gout"].to(DEV))
            torch.cuda.synchronize()
            info = launch_info()
        assert [r[0] for r in kt.records] == hd.FUSED_NAMES["levelref_masked"], kt.records
        assert_trips("big_u", info)
        got = [t.detach().cpu() for t in (out, v.grad, pr.grad, rf.grad)]
        assert not bool(got[1][~inp["mask"]].any())
        _assert_fused_close(got, inp, qm, pm, ac, f"fused_levelref both masks {pm} {int(ac)}")


def test_fused_ragged_with_a_query_mask():
    """per-level counts in the module's fused kernels under a query mask: the RaggedMaskedParams count and place passes"""
    from msda_triton_amd.functional import fused_module_core
    from test_gpu_module_masks import nothing_composed, spied_symbols
    B, Q, H, _, levels, counts = lp.BIG["big_c"][1]
    _assert_one_pass(sum(counts))
    inp = _draw("ragged", B, Q, H, levels, counts, 2, 102)
    qm = qmc.make_query_mask("bernoulli", B, Q, 4)
    for pm, ac in TWO_MODES:
        v, pr, rf = (inp[k].to(DEV).requires_grad_(True) for k in ("value", "proj", "ref"))
        log = []
        with options(value_path=2), nothing_composed(), spied_symbols(log):
            out = fused_module_core(v, inp["shapes"].to(DEV), pr, rf, pm, ac, None, counts, None, qm.to(DEV))
            out.backward(inp["gout"].to(DEV))
            torch.cuda.synchronize()
            info = launch_info()
        assert log == ["msda_fwd_fused_ragged_masked_f32", "msda_bwd_fused_ragged_masked_f32"], log
        assert_trips("big_c", info)
        got = [t.detach().cpu() for t in (out, v.grad, pr.grad, rf.grad)]
        _assert_fused_close(got, inp, qm, pm, ac, f"fused_ragged query mask {pm} {int(ac)}")


def test_fused_hfbox_discrete():
    """the box rule in front of discrete sampling against the composition on the same GPU (tests/test_gpu_hf_box_discrete.py)"""
    from msda_triton_amd.functional import KernelTimer
    from test_gpu_hf_box_discrete import assert_matches, only_the_fused_pair
    from test_gpu_hf_box_discrete import run as box_run
    from test_gpu_fused_ragged import names
    B, Q, H, _, levels, counts = lp.BIG["big_d"][1]
    _assert_one_pass(sum(counts))
    inp = _draw("hfbox", B, Q, H, levels, counts, 4, 103)
    c = [inp[k].to(DEV) for k in ("value", "shapes", "proj", "ref", "gout")]
    with options(value_path=2):
        with KernelTimer() as kt:
            got = box_run(True, *c, counts, 0.5)
            torch.cuda.synchronize()
        info = launch_info()
        want = box_run(False, *c, counts, 0.5)
        info_want = launch_info()
    assert only_the_fused_pair(kt), names(kt)
    assert info["fwd_variant"] == 4 and info["sample_variant"] == 3, info
    assert_trips("big_d", info)
    assert_trips("big_d", info_want)
    assert_matches(got, want)
