"""The exact-input fixtures of tests/exact_cases.py prove their own teeth on the CPU: the precondition holds for every
case tests/test_gpu_exact_numerics.py uses, the inputs survive 16-bit storage, the store really rounds, and emulated
wrong kernels (16-bit accumulation, a truncating store, a second rounding, coarse weights, a dropped corner) all differ
from `expected` — so a GPU kernel with one of those faults cannot pass the equality there."""
import numpy as np
import pytest
import torch

import exact_cases as ec
from exact_cases import BF16, F16, F32, MODES, TENSORS

MODE_IDS = [f"{pm}_{int(ac)}" for pm, ac in MODES]
SIXTEEN = [(n, dt) for n in ec.BILINEAR for dt in ec.storage_types(n)]
SIXTEEN_IDS = [f"{n}-{str(dt).split('.')[-1]}" for n, dt in SIXTEEN]
MIN_ROUNDED_SHARE = 0.05


def _t(a):
    return torch.from_numpy(np.array(a))


def _differs(mutant, want):
    assert mutant.shape == want.shape and mutant.dtype == want.dtype
    return not torch.equal(mutant, want)


# ----------------------------------------------------------------------------------------- the precondition
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ec.BILINEAR)
def test_precondition_holds(name, pm, ac):
    bud = ec.precondition(name, pm, ac)
    print(name, pm, ac, bud)
    assert set(bud) == set(TENSORS) and max(bud.values()) <= 24


@pytest.mark.parametrize("name", ec.DISCRETE)
def test_precondition_holds_discrete(name):
    bud = ec.precondition(name)
    print(name, bud)
    assert set(bud) == {"out", "grad_value", "grad_attn"} and max(bud.values()) <= 24


def test_a_case_outside_the_regime_fails_the_precondition():
    """The budget is not vacuous: the same generator with 11-bit locations needs more than 24 bits for `out`."""
    c = ec.exact_case(np.random.default_rng(0), 1, 5, 1, 4, [(9, 7)], 2, loc_bits=11, lo=0.0, hi=1.0)
    assert ec.budget(c, "zeros", False)["out"] > 24


@pytest.mark.parametrize("name", list(ec.CASES))
def test_inputs_survive_16_bit_storage(name):
    c = ec.get_case(name)
    for k in ("value", "loc", "attn", "grad_out"):
        t = _t(c[k])
        for dt in (F16, BF16, F32):
            assert torch.equal(t.to(dt).double(), t), (name, k, dt)


def test_generator_properties():
    c = ec.get_case("d8_vec_g4")  # (a case with the generator's defaults)
    k = c["loc"] * 128
    assert np.array_equal(k, np.round(k)) and (np.round(k).astype(np.int64) % 2 == 1).all()
    assert c["loc"].min() >= -0.3 and c["loc"].max() <= 1.3 and c["loc"].min() < 0 and c["loc"].max() > 1
    assert set(np.unique(c["attn"])) == {0.0, 0.25, 0.5, 0.75, 1.0}
    for key in ("value", "grad_out"):
        assert set(np.unique(c[key])) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    for name in ec.CASES:  # 0 and 1 among the weights of even the smallest case
        a = ec.get_case(name)["attn"]
        assert a.min() == 0.0 and a.max() == 1.0, name
    r = ec.get_case("ragged_125")
    assert r["loc"].shape == (2, 37, 2, 8, 2) and r["attn"].shape == (2, 37, 2, 8) and r["counts"] == [1, 2, 5]


@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
def test_flood_case_floods_one_cell_per_level(pm, ac):
    c = ec.get_case("flood")
    cell = np.floor(ec.pixel_coordinates(c, ac))
    for lvl, want in enumerate(((2, 2), (1, 1))):
        assert (cell[:, :, :, lvl] == np.asarray(want, dtype=np.float64)).all()
    assert c["loc"].shape[1] * c["loc"].shape[4] >= 2048  # samples per (plane, level), all in that cell


def test_numpy_formulation_is_the_oracle():
    """`contributions` (what the mutants below perturb) sums to the oracle's output, bitwise."""
    for name in ("d5_scalar", "many_levels", "ragged_363", "flood"):
        c = ec.get_case(name)
        for pm, ac in MODES:
            out = ec.contributions(c, pm, ac).sum(axis=(3, 4))
            assert np.array_equal(out, ec.reference(name, pm, ac)["out"]), (name, pm, ac)


# ----------------------------------------------------------------------------------------- the store really rounds
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,dt", SIXTEEN, ids=SIXTEEN_IDS)
def test_share_of_results_the_store_must_round(name, dt, pm, ac):
    """Per tensor, 16-bit case and mode: at least 5 % of the reference's elements are not representable in the storage
    type.  A condition on the inputs alone."""
    ref = ec.checked_reference(name, pm, ac)
    for k in TENSORS:
        share = float((ec.expected(ref[k], dt).double() != _t(ref[k])).double().mean())
        print(f"{name} {dt} {pm} {ac} {k}: {share:.1%} not representable")
        assert share >= MIN_ROUNDED_SHARE, (name, dt, pm, ac, k, share)


@pytest.mark.parametrize("name", ec.DISCRETE)
def test_share_of_results_the_store_must_round_discrete(name):
    ref = ec.checked_reference(name)
    for dt in ec.storage_types(name):
        for k, r in ref.items():
            share = float((ec.expected(r, dt).double() != _t(r)).double().mean())
            print(f"{name} {dt} {k}: {share:.1%} not representable")
            assert share >= MIN_ROUNDED_SHARE, (name, dt, k, share)
            assert _differs(ec.truncate(_t(r).float(), dt), ec.expected(r, dt)), (name, dt, k)


# ----------------------------------------------------------------------------------------- emulated wrong kernels
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name,dt", SIXTEEN, ids=SIXTEEN_IDS)
def test_16_bit_mutants_are_caught(name, dt, pm, ac):
    c = ec.get_case(name)
    ref = ec.checked_reference(name, pm, ac)
    want = ec.expected(ref["out"], dt)
    contrib = _t(ec.contributions(c, pm, ac)).float()  # [B, Q, H, L, P, D], exact in float32
    L, P = contrib.shape[3:5]
    # accumulating `out` in the storage type
    acc = torch.zeros(want.shape, dtype=dt)
    for lvl in range(L):
        for p in range(P):
            acc = (acc.float() + contrib[:, :, :, lvl, p]).to(dt)
    assert _differs(acc, want), "16-bit accumulation"
    # rounding twice: the partial sum goes through the storage type after each level (one level: after its first point)
    parts = [contrib[:, :, :, lvl].sum(3) for lvl in range(L)] if L > 1 else [contrib[:, :, :, 0, :1].sum(3),
                                                                              contrib[:, :, :, 0, 1:].sum(3)]
    acc = torch.zeros(want.shape, dtype=F32)
    for part in parts:
        acc = (acc + part).to(dt).float()
    assert _differs(acc.to(dt), want), "a rounding per partial sum"
    # a truncating store, on every tensor
    for k in TENSORS:
        assert _differs(ec.truncate(_t(ref[k]).float(), dt), ec.expected(ref[k], dt)), f"truncating store: {k}"


@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ec.BILINEAR)
def test_weight_mutants_are_caught_in_every_storage_type(name, pm, ac):
    c = ec.get_case(name)
    ref = ec.checked_reference(name, pm, ac)
    coarse = ec.contributions(c, pm, ac, weight_fn=lambda w: np.floor(w * 64.0) / 64.0).sum(axis=(3, 4))
    dropped = ec.contributions(c, pm, ac, drop=ec.smallest_corner_of_one_sample(c, pm, ac)).sum(axis=(3, 4))
    for dt in (F32,) + tuple(ec.storage_types(name)):
        want = ec.expected(ref["out"], dt)
        assert _differs(_t(coarse).float().to(dt), want), f"weights with 6 fractional bits, {dt}"
        assert _differs(_t(dropped).float().to(dt), want), f"smallest corner of one sample dropped, {dt}"
