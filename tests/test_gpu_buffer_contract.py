"""GPU: the buffer contract of every launcher family on benign inputs, through the guarded allocation rig
(tests/guarded_alloc.py).  Run with ``-m gpu``.

Each case runs three times — without the rig, with every allocation pre-filled 0xFF (NaN), with 0x5A — and must
  * leave every guard band intact (out, the gradients, the per-head grad_ref partials and the workspace),
  * be served exactly the allocations the launcher makes (a rig that was bypassed is a failure),
  * return bit-identical tensors in the three runs (every element written; nothing depends on what an output or the
    workspace held on entry), with no byte that still holds its pre-fill,
  * return finite tensors.
The calls go through the Python launchers (the native seam), never the C++ autograd node, which allocates in C++.
Shapes: the smallest at which each code path exists, taken from the suite's own tables."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

from guarded_alloc import GuardedAlloc, bits_equal, contract_violations
from msda_triton_amd import _lib, discrete, functional as F, ragged
from test_gpu_fused_ragged import COUNTS, SHAPES as FUSED_SHAPES
from test_gpu_lds_levels import CASES as LDS_CASES
from test_gpu_parity import DEV, SHAPE_MATRIX, rand_case
from test_gpu_value_mask import make_mask

pytestmark = pytest.mark.gpu

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
# name: (value / grad_value storage, storage of everything else) — the plain pair
STORAGE = {"f32": (F32, F32), "f64": (F64, F64), "fp16": (F16, F16), "bf16": (BF16, BF16), "f32_vbf16": (BF16, F32),
           "f32_vf16": (F16, F32)}
# name: (value and projection, reference points) — the fused families
FUSED_STORAGE = {"f32": (F32, F32), "f64": (F64, F64), "fp16": (F16, F16), "bf16": (BF16, BF16), "sbf16": (BF16, F32),
                 "sf16": (F16, F32)}
MODES = [("zeros", False), ("border", True)]

PLAIN_SHAPES = {k: SHAPE_MATRIX[k] for k in ("d32_vec_g8", "d5_scalar", "d8_vec_g4", "d1", "one_query",
                                             "d512_two_channel_chunks", "many_samples_chunked")}
PLAIN_SHAPES.update({k: LDS_CASES[k][:6] for k in ("c2_like_f32", "no_level_fits_but_last", "coarse_first_order", "bf16_g4",
                                                    "fp16_d64", "f64")})
# a partly filled lane group (17 of 32 lanes in float32; 16-bit: the scalar kernels' second chunk of 4 lanes) and a second
# channel chunk of ONE lane (16-bit: five scalar chunks) — d512_two_channel_chunks fills its lanes exactly
PLAIN_SHAPES["d68_partly_filled_group"] = (2, 11, 2, 68, [(5, 4), (3, 2)], 3)
PLAIN_SHAPES["d260_one_lane_second_chunk"] = (2, 11, 2, 260, [(5, 4), (3, 2)], 3)
# test_grad_value_without_workspace's pyramid: the sorted records' three homes (grad_loc, grad_attn, grad_value itself)
PLAIN_SHAPES["three_homes"] = (1, 2500, 2, 32, [(40, 40), (20, 20)], 2)

# allocations per call: out | grad_value, grad_loc, grad_attn, workspace | grad_value, grad_proj, grad_ref partials, workspace |
# (discrete) grad_value, grad_attn, workspace
N_FWD, N_BWD, N_BWD_FUSED, N_BWD_DISCRETE = 1, 4, 4, 3


@contextlib.contextmanager
def options(**kw):
    old = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def hold(call, n_alloc, what, names=None):
    """the three runs of one call; returns the rigs (for the allocation lists) and the plain results"""
    bad, rigs, results = contract_violations(call, n_alloc, DEV, names=names)
    assert not bad, (what, bad)
    return rigs, results[0]


def plain_inputs(name, storage, seed_salt=0, lo=-0.3, hi=1.3):
    B, Q, H, D, levels, P = PLAIN_SHAPES[name]
    vdt, cdt = STORAGE[storage]
    c = rand_case(np.random.default_rng(zlib.crc32(name.encode()) + seed_salt), B, Q, H, D, levels, P, lo=lo, hi=hi)
    v = torch.from_numpy(c["value"]).to(DEV, vdt)
    l, a, go = (torch.from_numpy(c[k]).to(DEV, cdt) for k in ("loc", "attn", "grad_out"))
    return v, torch.from_numpy(c["shapes"]).to(DEV), l, a, go


def plain_pair(v, s, l, a, go, pm, ac, what, mask=None):
    """forward and full backward of the plain pair (or its value-mask twin) under the contract; -> (rigs of the backward, results)"""
    out = hold(lambda: F.msda_hip_fwd(v, s, l, a, pm, ac, value_mask=mask), N_FWD, f"{what} fwd", ["out"])[1]
    rigs, grads = hold(lambda: F.msda_hip_bwd(go, v, s, l, a, pm, ac, value_mask=mask), N_BWD, f"{what} bwd",
                       ["grad_value", "grad_loc", "grad_attn"])
    assert out[0].shape == go.shape and grads[0].shape == v.shape and grads[1].shape == l.shape and grads[2].shape == a.shape
    assert grads[0].dtype == v.dtype and grads[1].dtype == l.dtype
    return rigs, out + grads


# ----------------------------------------------------------------------------------------- the plain pair and its masked twin
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "value_mask"])
@pytest.mark.parametrize("name", list(PLAIN_SHAPES))
def test_plain_pair_holds_the_buffer_contract(name, masked):
    B, levels = PLAIN_SHAPES[name][0], PLAIN_SHAPES[name][4]
    mask = make_mask("bernoulli", B, levels, zlib.crc32(name.encode())).to(DEV) if masked else None
    for storage in STORAGE:
        v, s, l, a, go = plain_inputs(name, storage)
        for pm, ac in MODES:
            plain_pair(v, s, l, a, go, pm, ac, f"{name} {storage} {pm}/{ac} masked={masked}", mask)


# (route, options, expected launch info) — every forced route is confirmed through last_launch_info
ROUTES = {
    "sorted_records_in_ws": ("d32_vec_g8", dict(value_path=2, records_in_grads=0), dict(value_path=2)),
    "sorted_records_in_grads": ("d32_vec_g8", dict(value_path=2, records_in_grads=1), dict(value_path=2)),
    "single_launch_rig0": ("c2_like_f32", dict(value_path=3, records_in_grads=0), dict(value_path=1)),
    "single_launch_rig1": ("c2_like_f32", dict(value_path=3, records_in_grads=1), dict(value_path=1)),
    "sorted_c2_like_rig0": ("c2_like_f32", dict(value_path=2, records_in_grads=0), dict(value_path=2)),
    "sorted_c2_like_rig1": ("c2_like_f32", dict(value_path=2, records_in_grads=1), dict(value_path=2)),
    "three_homes_rig0": ("three_homes", dict(records_in_grads=0), dict(value_path=2)),
    "three_homes_rig1": ("three_homes", dict(records_in_grads=1), dict(value_path=2)),
    "two_passes": ("d32_vec_g8", dict(value_path=2, ws_passes=2), dict(value_path=2, value_passes=2)),
    "two_passes_c2_like": ("c2_like_f32", dict(value_path=2, ws_passes=2), dict(value_path=2, value_passes=2)),
    "rounds_of_7_queries": ("d32_vec_g8", dict(value_path=2, q_round=7), dict(value_path=2)),
    "unit_fwd_off": ("d32_vec_g8", dict(unit_fwd=0, lds_levels=0), dict(fwd_variant=0)),
    "unit_fwd_forced": ("d32_vec_g8", dict(unit_fwd=2), dict(fwd_variant=2)),
    "unit_fwd_forced_c2_like": ("c2_like_f32", dict(unit_fwd=2), dict(fwd_variant=2)),
}


@pytest.mark.parametrize("storage", ["f32", "f64", "fp16", "bf16"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_forced_routes_hold_the_buffer_contract(route, storage):
    name, opts, want = ROUTES[route]
    v, s, l, a, go = plain_inputs(name, storage, seed_salt=1, lo=-0.05, hi=1.05)
    ws_bytes = {}
    with options(**opts):
        for pm, ac in MODES:
            rigs, _ = plain_pair(v, s, l, a, go, pm, ac, f"{route} {storage} {pm}/{ac}")
            info = _lib.last_launch_info()
            for k, val in want.items():
                if k == "fwd_variant" and val == 2 and storage == "f64":
                    # the one-wave-per-unit forward exists for 16-byte vectors with float arithmetic only: f64 keeps the general kernel
                    assert info[k] in (0, 1), (route, storage, k, info)
                    continue
                assert info[k] == val, (route, storage, k, info)
            ws_bytes[pm] = rigs[0].allocations[3]["bytes"]
            assert rigs[0].allocations[3]["dtype"] == torch.uint8 and rigs[1].allocations[3]["bytes"] == ws_bytes[pm]
    if want.get("value_path") == 1:
        assert set(ws_bytes.values()) == {0}, ws_bytes  # the single-launch kernel: its index lives in LDS
    elif want.get("value_path") == 2:
        assert min(ws_bytes.values()) > 0, ws_bytes


@pytest.mark.parametrize("name", ["d32_vec_g8", "c2_like_f32", "three_homes"])
def test_records_in_grads_takes_the_records_out_of_the_workspace(name):
    """the route `records_in_grads` names has no launch-info key: it shows in the workspace the launcher asks the rig for"""
    v, s, l, a, go = plain_inputs(name, "f32", seed_salt=2, lo=-0.05, hi=1.05)
    Q, L, P = l.shape[1], l.shape[3], l.shape[4]
    size, grads = {}, {}
    for rig_opt in (0, 1):
        with options(value_path=2, records_in_grads=rig_opt):
            rigs, res = plain_pair(v, s, l, a, go, "zeros", False, f"{name} records_in_grads={rig_opt}")
            assert _lib.last_launch_info()["value_path"] == 2
        size[rig_opt], grads[rig_opt] = rigs[0].allocations[3]["bytes"], res
    assert 0 < size[1] < size[0], size
    if name == "three_homes":
        assert size[1] <= size[0] - 2 * Q * L * P * 16, size  # both planes' 16-byte records are gone from it
    for x, y in zip(grads[0], grads[1]):  # same records, same order, wherever they were kept
        assert bits_equal(x, y)


@pytest.mark.parametrize("storage", ["f32", "f32_vbf16"])  # (float arithmetic on 16-byte pieces: the LDS variants' types)
@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("lds", [0, 2])
@pytest.mark.parametrize("name", ["c2_like_f32", "no_level_fits_but_last", "coarse_first_order"])
def test_lds_served_levels_hold_the_buffer_contract(name, lds, planes, storage):
    v, s, l, a, go = plain_inputs(name, storage, seed_salt=3)
    with options(unit_fwd=0, lds_levels=lds, lds_planes=planes):
        for pm, ac in MODES:
            plain_pair(v, s, l, a, go, pm, ac, f"{name} lds_levels={lds} lds_planes={planes} {storage} {pm}/{ac}")
            info = _lib.last_launch_info()
            if lds == 0:
                assert info["fwd_variant"] == 0 and info["sample_variant"] == 0 and info["fwd_lds_level_bytes"] == 0, info
            else:
                assert info["fwd_variant"] == 1 and info["fwd_lds_level_bytes"] > 0 and info["sample_variant"] == 1, info
                assert info["fwd_lds_planes"] in (1, planes), info
                if name == "c2_like_f32":  # (H = 4: neighbouring heads share a workgroup)
                    assert info["fwd_lds_planes"] == planes, info


@pytest.mark.parametrize("storage", ["f64", "fp16", "bf16"])
@pytest.mark.parametrize("lds,planes", [(2, 1), (2, 2)])
def test_lds_options_on_types_without_the_variant(lds, planes, storage):
    """f64 and pure 16-bit storage have no LDS-served kernels: the options must leave their buffers alone all the same"""
    v, s, l, a, go = plain_inputs("c2_like_f32", storage, seed_salt=3)
    with options(unit_fwd=0, lds_levels=lds, lds_planes=planes):
        for pm, ac in MODES:
            plain_pair(v, s, l, a, go, pm, ac, f"lds_levels={lds} lds_planes={planes} {storage} {pm}/{ac}")
            assert _lib.last_launch_info()["fwd_variant"] in (0, 1)


# ----------------------------------------------------------------------------------------- the fused families, uniform counts
def fused_uniform_inputs(name, storage, levelref, ref_dim):
    B, Q, H, D, levels, P = PLAIN_SHAPES[name]
    sdt, rdt = FUSED_STORAGE[storage]
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(name.encode()) + ref_dim)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g)
    proj = torch.randn(B, Q, H, len(levels), P, 3, generator=g) * 1.5
    ref = torch.rand(*((B, Q, len(levels), ref_dim) if levelref else (B, Q, ref_dim)), generator=g)
    gout = torch.rand(B, Q, H, D, generator=g)
    return value.to(DEV, sdt), torch.tensor(levels, device=DEV), proj.to(DEV, sdt), ref.to(DEV, rdt), gout.to(DEV, sdt)


def fused_pair(fwd, bwd, what, n_bwd=N_BWD_FUSED):
    out = fwd()
    if out is None:
        return None  # (the library declined: the caller checks that it had to)
    hold(fwd, N_FWD, f"{what} fwd", ["out"])
    rigs, _ = hold(bwd, n_bwd, f"{what} bwd", ["grad_value", "grad_proj", "grad_ref"])
    return rigs


@pytest.mark.parametrize("kind", ["uniform", "levelref", "levelref_masked"])
@pytest.mark.parametrize("name", list(PLAIN_SHAPES))
def test_fused_uniform_families_hold_the_buffer_contract(name, kind):
    B, Q, H, D, levels, P = PLAIN_SHAPES[name]
    levelref = kind != "uniform"
    mask = make_mask("bernoulli", B, levels, zlib.crc32(name.encode())).to(DEV) if kind == "levelref_masked" else None
    storages = ["f32", "f64", "fp16", "bf16"] + (["sbf16", "sf16"] if name == "d32_vec_g8" else [])
    for storage in storages:
        for (pm, ac), ref_dim in zip(MODES, (2, 4)):
            v, s, pr, rf, go = fused_uniform_inputs(name, storage, levelref, ref_dim)
            kw = dict(levelref=levelref, value_mask=mask) if levelref else {}
            rigs = fused_pair(lambda: F.msda_hip_fwd_fused(v, s, pr, rf, pm, ac, **kw),
                              lambda: F.msda_hip_bwd_fused(go, v, s, pr, rf, pm, ac, **kw), f"{name} {kind} {storage} {pm}/{ac}")
            if rigs is None:  # only the shape whose L * P samples do not fit one LDS pass may be declined
                limit = int(_lib.load().msda_fused_lp_limit(D, 4 if storage in ("sbf16", "sf16") else pr.element_size()))
                assert len(levels) * P > limit, (name, storage, limit)
                continue
            part = rigs[0].allocations[2]  # the per-head grad_ref partials: banded like the rest
            assert part["shape"] == ((B, Q, H, len(levels), ref_dim) if levelref else (B, Q, H, ref_dim)) and part["dtype"] == rf.dtype


# ----------------------------------------------------------------------------------------- per-level point counts
def ragged_inputs(sname, cname, storage, ref_dim):
    B, Q, H, D, levels = FUSED_SHAPES[sname]
    counts = tuple(COUNTS[cname])
    levels = levels[:len(counts)]
    sdt, rdt = FUSED_STORAGE[storage]
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{sname}{cname}".encode()) + ref_dim)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g)
    proj = torch.randn(B, Q, H, sum(counts), 3, generator=g) * 1.5
    ref = torch.rand(B, Q, ref_dim, generator=g)
    gout = torch.rand(B, Q, H, D, generator=g)
    return value.to(DEV, sdt), torch.tensor(levels, device=DEV), proj.to(DEV, sdt), ref.to(DEV, rdt), gout.to(DEV, sdt), counts


def declined(v, pr, counts, storage, what):
    """the library may decline a fused call only when a unit's S samples do not fit one LDS pass (f64 at D = 8: 9 samples)"""
    limit = int(_lib.load().msda_fused_lp_limit(v.shape[3], 4 if storage in ("sbf16", "sf16") else pr.element_size()))
    assert sum(counts) > limit, (what, limit)
    return None


def one_ragged_family(family, sname, cname, storage, pm, ac, ref_dim):
    v, s, pr, rf, go, counts = ragged_inputs(sname, cname, storage, 4 if family == "hf_box_fused" else ref_dim)
    what = f"{family} {sname} {cname} {storage} {pm}/{ac}"
    if family == "ragged_fused":
        rigs = fused_pair(lambda: ragged.ragged_hip_fwd_fused(v, s, pr, rf, pm, ac, counts),
                          lambda: ragged.ragged_hip_bwd_fused(go, v, s, pr, rf, pm, ac, counts), what)
        return rigs if rigs is not None else declined(v, pr, counts, storage, what)
    if family == "hf_box_fused":
        rigs = fused_pair(lambda: ragged.hf_box_hip_fwd_fused(v, s, pr, rf, pm, ac, counts),
                          lambda: ragged.hf_box_hip_bwd_fused(go, v, s, pr, rf, pm, ac, counts), what)
        return rigs if rigs is not None else declined(v, pr, counts, storage, what)
    # the unfused operators: sampling points and weights from the module's prologue, in the arithmetic dtype
    pts, att = ragged.ragged_module_sampling_inputs(pr.to(rf.dtype), s, rf, counts)
    pts, att, go = pts.contiguous(), att.contiguous(), go.to(rf.dtype)
    if family == "ragged":
        hold(lambda: ragged.ragged_hip_fwd(v, s, pts, att, pm, ac, counts), N_FWD, f"{what} fwd", ["out"])
        return hold(lambda: ragged.ragged_hip_bwd(go, v, s, pts, att, pm, ac, counts), N_BWD, f"{what} bwd",
                    ["grad_value", "grad_loc", "grad_attn"])[0]
    assert family == "discrete"
    hold(lambda: discrete.discrete_hip_fwd(v, s, pts, att, counts), N_FWD, f"{what} fwd", ["out"])
    return hold(lambda: discrete.discrete_hip_bwd(go, v, s, pts, att, counts), N_BWD_DISCRETE, f"{what} bwd",
                ["grad_value", "grad_attn"])[0]


RAGGED_FAMILIES = ["ragged", "ragged_fused", "hf_box_fused", "discrete"]


@pytest.mark.parametrize("cname", list(COUNTS))
@pytest.mark.parametrize("sname", list(FUSED_SHAPES))
@pytest.mark.parametrize("family", RAGGED_FAMILIES)
def test_per_level_count_families_hold_the_buffer_contract(family, sname, cname):
    storages = ["f32", "f64", "fp16", "bf16"]
    if sname == "d32" and cname == "3_6_3":  # one shape per family in the module's 16-bit storage (the unfused operators:
        storages += ["sbf16", "sf16"]        # a 16-bit value next to fp32 sampling inputs, f32_vbf16 / f32_vf16)
    for storage in storages:
        for (pm, ac), ref_dim in zip(MODES, (2, 4)):
            if family == "discrete" and (pm, ac) != ("border", True):
                continue  # (no padding mode: one run)
            one_ragged_family(family, sname, cname, storage, pm, ac, ref_dim)


@pytest.mark.parametrize("family", RAGGED_FAMILIES)
def test_per_level_count_families_on_both_grad_value_routes(family):
    for value_path, want in ((2, 2), (3, 1)):
        for rig_opt in (0, 1):
            with options(value_path=value_path, records_in_grads=rig_opt):
                one_ragged_family(family, "d32", "3_6_3", "f32", "zeros", False, 4)
                assert _lib.last_launch_info()["value_path"] == want, (family, value_path)
    with options(value_path=2, ws_passes=2, q_round=7):
        one_ragged_family(family, "d32", "2_4_6_4", "bf16", "border", True, 2)
        info = _lib.last_launch_info()
        assert info["value_path"] == 2 and info["value_passes"] == 2, (family, info)


# ----------------------------------------------------------------------------------------- degenerate calls
def test_degenerate_calls_through_the_rig():
    """Q = 0, no points, no pixels' worth of samples: the launchers answer with memsets (or nothing) — of the right size"""
    s = torch.tensor([[3, 3]], device=DEV)
    v = torch.randn(2, 9, 2, 8, device=DEV)
    for Q, P in ((0, 2), (5, 0), (0, 0)):
        l, a, go = torch.rand(2, Q, 2, 1, P, 2, device=DEV), torch.rand(2, Q, 2, 1, P, device=DEV), torch.rand(2, Q, 2, 8, device=DEV)
        for mask in (None, make_mask("bernoulli", 2, [(3, 3)], 1).to(DEV)):
            _, res = plain_pair(v, s, l, a, go, "zeros", False, f"Q={Q} P={P}", mask)
            assert res[0].shape == (2, Q, 2, 8) and all(int(torch.count_nonzero(t)) == 0 for t in res)
        pr, rf = torch.randn(2, Q, 2, 1, P, 3, device=DEV), torch.rand(2, Q, 2, device=DEV)
        fwd = lambda: F.msda_hip_fwd_fused(v, s, pr, rf, "border", True)  # noqa: E731
        assert fwd() is not None
        _, res = hold(fwd, N_FWD, f"fused fwd Q={Q} P={P}")
        assert int(torch.count_nonzero(res[0])) == 0
        _, res = hold(lambda: F.msda_hip_bwd_fused(go, v, s, pr, rf, "border", True), N_BWD_FUSED, f"fused bwd Q={Q} P={P}")
        assert all(int(torch.count_nonzero(t)) == 0 for t in res)
        # the other fused families share run_bwd_fused's shortcut: per-level reference points (and the mask twin) here,
        # the per-level-count pair and the box rule below
        rl = torch.rand(2, Q, 1, 4, device=DEV)
        for mask in (None, make_mask("bernoulli", 2, [(3, 3)], 1).to(DEV)):
            kw = dict(levelref=True, value_mask=mask)
            _, res = hold(lambda: F.msda_hip_fwd_fused(v, s, pr, rl, "zeros", False, **kw), N_FWD, f"levelref fwd Q={Q} P={P}")
            assert res[0].shape == (2, Q, 2, 8) and int(torch.count_nonzero(res[0])) == 0
            _, res = hold(lambda: F.msda_hip_bwd_fused(go, v, s, pr, rl, "zeros", False, **kw), N_BWD_FUSED,
                          f"levelref bwd Q={Q} P={P}")
            assert res[2].shape == (2, Q, 1, 4) and all(int(torch.count_nonzero(t)) == 0 for t in res)
        if P == 0:
            continue  # (per-level counts: every level needs at least one point)
        counts = (P,)
        pts, att = l.reshape(2, Q, 2, P, 2), a.reshape(2, Q, 2, P)
        prr, box = pr.reshape(2, Q, 2, P, 3), torch.rand(2, Q, 4, device=DEV)
        for fam_fwd, fam_bwd, n in (
                (lambda: ragged.ragged_hip_fwd_fused(v, s, prr, rf, "border", True, counts),
                 lambda: ragged.ragged_hip_bwd_fused(go, v, s, prr, rf, "border", True, counts), N_BWD_FUSED),
                (lambda: ragged.hf_box_hip_fwd_fused(v, s, prr, box, "zeros", False, counts),
                 lambda: ragged.hf_box_hip_bwd_fused(go, v, s, prr, box, "zeros", False, counts), N_BWD_FUSED),
                (lambda: ragged.ragged_hip_fwd(v, s, pts, att, "zeros", False, counts),
                 lambda: ragged.ragged_hip_bwd(go, v, s, pts, att, "zeros", False, counts), N_BWD),
                (lambda: discrete.discrete_hip_fwd(v, s, pts, att, counts),
                 lambda: discrete.discrete_hip_bwd(go, v, s, pts, att, counts), N_BWD_DISCRETE)):
            assert fam_fwd() is not None and fam_bwd() is not None  # (a fused pair must not decline these)
            _, res = hold(fam_fwd, N_FWD, f"fwd Q={Q} P={P}")
            assert int(torch.count_nonzero(res[0])) == 0
            _, res = hold(fam_bwd, n, f"bwd Q={Q} P={P}")
            assert all(int(torch.count_nonzero(t)) == 0 for t in res)


# ----------------------------------------------------------------------------------------- caller-owned buffers
PATTERN = 0x5A


def _slab(rows, row_shape, dtype, lo, hi):
    """a [rows, *row_shape] tensor of PATTERN bytes and its rows lo .. hi as one contiguous buffer"""
    t = torch.empty((rows,) + tuple(row_shape), dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(PATTERN)
    return t, t[lo:hi]


def _neighbours_untouched(t, lo, hi):
    b = t.view(torch.uint8)
    return bool((b[:lo] == PATTERN).all()) and bool((b[hi:] == PATTERN).all())


@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vf16"])
@pytest.mark.parametrize("name,opts", [("d32_vec_g8", dict(value_path=2)), ("d32_vec_g8", dict(value_path=3)),
                                       ("d5_scalar", {}), ("three_homes", {})],
                         ids=["d32_sorted", "d32_single_launch", "d5_scalar", "three_homes"])
def test_out_buffers_that_are_slices_of_a_gather_buffer(name, opts, storage):
    """`out=`: interior slices of one tensor whose rows on either side (other ranks' results) hold a pattern"""
    v, s, l, a, go = plain_inputs(name, storage, seed_salt=4, lo=-0.05, hi=1.05)
    B = v.shape[0]
    with options(**opts):
        want_out = F.msda_hip_fwd(v, s, l, a, "zeros", False)
        want = F.msda_hip_bwd(go, v, s, l, a, "zeros", False)
        # three "ranks" of B batch elements each: this call owns the middle one
        gather, mine = _slab(3 * B, want_out.shape[1:], want_out.dtype, B, 2 * B)
        got_out = F.msda_hip_fwd(v, s, l, a, "zeros", False, out=mine)
        slabs = [_slab(3 * B, w.shape[1:], w.dtype, B, 2 * B) for w in want]
        got = F.msda_hip_bwd(go, v, s, l, a, "zeros", False, out=tuple(m for _, m in slabs))
        torch.cuda.synchronize()
    assert got_out.data_ptr() == mine.data_ptr() and bits_equal(got_out, want_out)
    assert _neighbours_untouched(gather, B, 2 * B), "out"
    for nm, (slab, m), g, w in zip(("grad_value", "grad_loc", "grad_attn"), slabs, got, want):
        assert g.data_ptr() == m.data_ptr() and bits_equal(g, w), nm
        assert _neighbours_untouched(slab, B, 2 * B), nm


# ----------------------------------------------------------------------------------------- the tests can fail
def test_a_wrong_expectation_and_a_short_buffer_are_caught():
    """The one negative case on the GPU (the mutants live in tests/test_guarded_alloc.py): the harness reports a call whose
    allocation count is not the launcher's, a comparison against a wrong expectation differs, and an `out=` buffer one row
    short of the launcher's shape check — the rig's own interior — raises ValueError before anything is launched: the
    interior keeps its pre-fill and the bands their pattern."""
    v, s, l, a, go = plain_inputs("d32_vec_g8", "f32", seed_salt=5)
    bad, _, results = contract_violations(lambda: F.msda_hip_bwd(go, v, s, l, a, "zeros", False), N_BWD + 1, DEV)
    assert len(bad) == 2 and all(f"served {N_BWD} allocations, the launcher makes {N_BWD + 1}" in b for b in bad), bad
    wrong = results[0][0].clone()
    wrong[-1, -1, -1, -1] = torch.nextafter(wrong[-1, -1, -1, -1], torch.tensor(float("inf"), device=DEV))  # one ulp, last row
    assert not bits_equal(results[1][0], wrong) and bits_equal(results[1][0], results[0][0])
    B, I, H, D = v.shape
    with GuardedAlloc(0xFF, DEV) as rig:
        short = torch.empty((B, I - 1, H, D), dtype=v.dtype, device=DEV)
        with pytest.raises(ValueError):
            F.msda_hip_bwd(go, v, s, l, a, "zeros", False, out=(short, None, None))
    torch.cuda.synchronize()
    assert len(rig.served) == 1  # nothing else was allocated, nothing launched
    assert bool(torch.isnan(short).all()) and not rig.band_violations()
