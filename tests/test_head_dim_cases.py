"""The head-dimension sweep proves on the CPU that it reaches what it claims: for every storage type the list of head
dimensions covers every required (path, G / chunks / partly filled) class of tests/head_dim_cases.py, and every case of
tests/test_gpu_head_dim.py is exact in float32 (tests/exact_cases.py: budget <= 24 bits, float32 oracle == float64
oracle, no sample on a grid kink) with a 16-bit store that really rounds."""
import numpy as np
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
from exact_cases import BF16, MODES, TENSORS

MODE_IDS = [f"{pm}_{int(ac)}" for pm, ac in MODES]
BILINEAR = [n for n in ec.HEAD_DIM if ec.CASES[n][0] == "bilinear"]
DISCRETE = [n for n in ec.HEAD_DIM if ec.CASES[n][0] == "discrete"]


def test_pick_group_and_vec_rule():
    assert [hd.pick_group(n) for n in (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64, 64]
    assert hd.instantiation("f32", 36) == (4, 16, 1)   # 36 % 4 == 0: nine 16-byte lanes, not the scalar path
    assert hd.instantiation("f32", 33) == (1, 64, 1)
    assert hd.instantiation("f32", 68) == (4, 32, 1) and hd.partly_filled("f32", 68)     # 17 of 32 lanes
    assert hd.instantiation("f32", 260) == (4, 64, 2) and hd.partly_filled("f32", 260)   # a second chunk of one lane
    assert hd.instantiation("f32", 256) == (4, 64, 1) and not hd.partly_filled("f32", 256)
    assert hd.instantiation("f32", 260, aligned=False) == (1, 64, 5)
    assert hd.instantiation("bf16", 72) == (8, 16, 1) and hd.instantiation("bf16", 68) == (1, 64, 2)
    assert hd.instantiation("f32_vbf16", 68) == (4, 32, 1)   # mixed storage computes in float32
    assert hd.instantiation("f64", 34) == (2, 32, 1) and hd.instantiation("f64", 260) == (2, 64, 3)


@pytest.mark.parametrize("storage", hd.STORAGES)
def test_head_dims_reach_every_required_class(storage):
    got, need = hd.classes(storage), hd.required(storage)
    print(storage, sorted(got))
    assert need <= got, (storage, sorted(need - got))
    if storage != "f64":  # (f64's scalar path: D = 130 is even, so it takes 16-byte pieces there)
        assert ("scalar", "chunks3+") in got
    assert ("vec", "chunks3+") in got or storage in hd.SIXTEEN_BIT


def test_every_head_dim_has_its_cases_on_the_base_shape():
    B, Q, H, levels = ec.HEAD_DIM_BASE
    for D in hd.HEAD_DIMS:
        for kind, P in (("p3", 3), ("c25", [2, 5]), ("disc", [2, 5])):
            assert ec.CASES[hd.case_name(D, kind)][1] == (B, Q, H, D, levels, P)
    assert Q % 4 and B * H > 1 and len(levels) == 2  # a last workgroup that is not full at every G; planes; levels


def test_forced_variant_tables_follow_the_launcher_rules():
    for (storage, D), variant in hd.UNIT_FWD.items():
        vec, _, _ = hd.instantiation(storage, D)
        lanes = D // vec
        takes = storage != "f64" and vec * hd.ARITH_BYTES[storage] == 16 and D % vec == 0 and lanes <= hd.WAVE and lanes & (lanes - 1) == 0
        assert variant == (2 if takes else 0), (storage, D)
    for (storage, D), (fwd, sample) in hd.LDS_LEVELS.items():
        vec, g, _ = hd.instantiation(storage, D)
        assert fwd == int(vec == 4 and g <= 16) and sample == int(vec == 4 and g <= 8), (storage, D)
    assert {hd.instantiation(s, D)[1] for s, D in hd.LDS_LEVELS} == {32, 64}
    assert {D // hd.instantiation(s, D)[0] for (s, D), v in hd.UNIT_FWD.items() if v == 2} == {32, 64}


@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", BILINEAR)
def test_precondition_holds(name, pm, ac):
    bud = ec.precondition(name, pm, ac)
    print(name, pm, ac, bud)
    assert set(bud) == set(TENSORS) and max(bud.values()) <= 24
    # the bf16 store has teeth: a fifth of `out` and of grad_value is not representable (grad_loc: values and gradients of
    # +-1 leave it short sums, so only that it rounds at all; float16's 11 bits hold most of these numbers)
    ref = ec.reference(name, pm, ac)
    share = {k: float((ec.expected(ref[k], BF16).double() != torch.from_numpy(ref[k])).double().mean()) for k in TENSORS}
    print(share)
    assert share["out"] >= 0.2 and share["grad_value"] >= 0.15 and share["grad_attn"] >= 0.05 and share["grad_loc"] > 0


@pytest.mark.parametrize("name", DISCRETE)
def test_precondition_holds_discrete(name):
    bud = ec.precondition(name)
    assert set(bud) == {"out", "grad_value", "grad_attn"} and max(bud.values()) <= 24
    for k, r in ec.reference(name).items():
        share = float((ec.expected(r, BF16).double() != torch.from_numpy(np.array(r))).double().mean())
        assert share >= 0.05, (name, k, share)


# ----------------------------------------------------------------------------------------- the fused families
def test_fused_lp_limit_restated():
    from msda_triton_amd import _lib
    lib = _lib.load()  # (host code: no GPU needed)
    for D in sorted(set(hd.HEAD_DIMS) | {8, 32, 64, 128, 256}):
        for elem in (2, 4, 8):
            assert hd.fused_lp_limit(D, elem) == int(lib.msda_fused_lp_limit(D, elem)), (D, elem)
    assert hd.fused_lp_limit(64, 4) < hd.FUSED_LARGE <= hd.fused_lp_limit(68, 4)  # G = 16 holds 68 samples, G = 32 138


@pytest.mark.parametrize("storage", list(hd.FUSED_DIMS))
def test_fused_dims_reach_every_class(storage):
    arith = hd.FUSED_ARITH[storage]
    cases = [(D, S) for f, s, D, S in hd.fused_case_list() if f == "uniform" and s == storage]
    assert {c for c in hd.fused_case_list() if c[0] == "uniform"} == {("uniform",) + c[1:] for c in hd.fused_case_list() if c[0] == "hfbox"}
    got = hd.classes(arith, [D for D, _ in cases])
    need = {("vec", "g32"), ("vec", "g64"), ("vec", "chunks2+"), ("vec", "partial"), ("scalar", "g64")}
    if storage in ("f32", "f64", "bf16", "fp16"):
        need |= hd.required(arith)
    assert need <= got, (storage, sorted(need - got))
    # more samples than lanes (the lane-strided softmax): at G = 32 and G = 64, one chunk and several, on both paths where
    # the one-pass limit admits 70 samples at all (fused_case_list)
    large = {hd.instantiation(arith, D) for D, S in cases if S == hd.FUSED_LARGE}
    assert all(S <= hd.fused_lp_limit(D, hd.fused_elem_size(storage)) for D, S in cases)
    assert {g for _, g, _ in large} >= {32, 64} and any(c > 1 for _, _, c in large)
    if storage in ("f32", "f64", "bf16", "fp16"):
        assert any(v == 1 for v, _, _ in large)


@pytest.mark.parametrize("family,storage,D,S", [c for c in hd.fused_case_list() if c[1] in hd.FUSED_AGAINST_FP64],
                         ids=[f"{f}-{s}-d{d}-s{n}" for f, s, d, n in hd.fused_case_list() if s in hd.FUSED_AGAINST_FP64])
def test_fused_kink_share_is_under_the_cap(family, storage, D, S):
    """From the reference alone: the share of offset gradients the GPU test compares away from grid kinks (in fact none:
    the draws are kink-free, because the reference points' gradients cannot be masked sample by sample)."""
    for ref_dim in hd.fused_ref_dims(family):
        inp = hd.fused_inputs(family, storage, D, S, ref_dim)
        assert not inp["proj"].requires_grad and inp["proj"].shape[:3] == (2, 11, 2)
        for _, ac in hd.FUSED_MODES:
            k = hd.fused_kinks(inp, ac)
            assert k.shape == inp["proj"][..., :2].shape
            assert float(k.mean()) <= hd.KINK_CAP and not k.any()
