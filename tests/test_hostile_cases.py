"""CPU preconditions of tests/test_gpu_hostile_inputs.py: what that file expects of the kernels on hostile sampling
inputs is a property of the OPERATION — the oracle (which clamps in floating point before any conversion) and the host
path show it without a GPU — and the case builders of tests/hostile_cases.py keep their promises."""
import numpy as np
import pytest
import torch

import hostile_cases as hc
from conftest import MODES, kink_mask, mode_key
from test_gpu_parity import BWD_TOL, FWD_TOL

F32 = torch.float32
NAMES = list(hc.plain_shapes())
TENSORS = ("out", "grad_value", "grad_loc", "grad_attn")


def run_oracle(oracle, c, pm, ac, dtype):
    a = {k: (v if k == "shapes" else v.astype(dtype)) for k, v in c.items()}
    out = oracle.forward(a["value"], a["shapes"], a["loc"], a["attn"], pm, ac)
    gv, gl, ga = oracle.backward(a["grad_out"], a["value"], a["shapes"], a["loc"], a["attn"], pm, ac)
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_attn=ga)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def native_forward(c, pm, ac):
    from msda_triton_amd.functional import native_multiscale_deformable_attention
    t = {k: torch.from_numpy(v) for k, v in c.items()}
    return native_multiscale_deformable_attention(t["value"], t["shapes"], t["loc"], t["attn"], pm, ac).numpy()


@pytest.mark.parametrize("name", NAMES)
def test_builders_keep_the_cap_and_touch_batch_element_0_only(name):
    c, hq, storage = hc.plain_case(name)
    Q = c["loc"].shape[1]
    assert c["loc"].shape[0] >= 2 and 1 <= len(hq) <= hc.MAX_HOSTILE_FRACTION * Q and len(set(hq.tolist())) == len(hq)
    far = hc.far_case(c, hq, storage)
    clean = hc.check_plant(far, c, hq)
    assert clean.sum() == Q - len(hq) and not hc.classify(far, storage).any()
    assert (far["loc"][0][hq] != c["loc"][0][hq]).any()
    for vname, v in hc.NONFINITE.items():
        for where in ("loc", "attn"):
            nf, planted = hc.nonfinite_case(c, hq, v, where)
            hc.check_plant(nf, c, hq)
            bad = hc.classify(nf, storage)
            assert bad[0][hq].all() and not bad[0][clean].any() and not bad[1:].any(), (vname, where)
            neutral = hc.neutralised(nf, planted)
            assert np.isfinite(neutral["loc"]).all() and np.isfinite(neutral["attn"]).all()
            if where == "loc":  # x only, y only and both all occur, next to samples left benign
                x_bad, y_bad = (~np.isfinite(nf["loc"][0][hq][..., i]) for i in (0, 1))
                assert (x_bad & ~y_bad).any() and (~x_bad & y_bad).any() and (x_bad & y_bad).any() and (~x_bad & ~y_bad).any()
    with pytest.raises(AssertionError):
        hc.hostile_queries(3)


def test_far_values_hit_the_wrap_marks_and_the_amp_case_overflows():
    for n in (16, 8, 4, 2):
        vals = hc.far_values(n)
        for k in hc.WRAP_EXPONENTS:
            with np.errstate(over="ignore"):
                assert any(np.float32(v) * np.float32(n) == np.float32(2.0 ** k) for v in vals), (n, k)  # exactly on the mark
    assert all(np.isfinite(np.float32(v)) for v in hc.far_values(16))
    # float16 storage: the AMP case — finite float32 values that become +-Inf on the cast
    c, hq, _ = hc.plain_case("fp16_d64")
    amp = hc.overflow_case(c, hq, torch.float16)
    bad16, bad64 = hc.classify(amp, torch.float16), hc.classify(amp, torch.float64)
    assert bad16[0][hq].all() and not bad16[1:].any() and not bad64.any()
    assert bool(torch.isinf(torch.from_numpy(amp["loc"]).to(torch.float16)[0]).any())
    for storage in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert not hc.classify(hc.far_case(c, hq, storage), storage).any()  # what stays FAR in a storage type is finite in it
    # float32 arithmetic: +-3.0e38 is finite, its pixel coordinate 3.0e38 * w is not (w >= 2) — and nothing else leaves FAR
    c, hq, _ = hc.plain_case("d32_vec_g8")
    over = hc.overflow_case(c, hq, torch.float32)
    changed = over["loc"][0][hq][over["loc"][0][hq] != c["loc"][0][hq]]
    assert set(np.abs(changed).tolist()) == {float(np.float32(3.0e38))} and np.isfinite(over["loc"]).all()
    assert hc.classify(over, torch.float32)[0][hq].all() and not hc.classify(over, torch.float64).any()
    for n in (16, 8, 4, 2):
        kept = [v for v in hc.far_values(n) if hc.stays_far(v, n, torch.float32)]
        assert sorted(set(hc.far_values(n)) - set(kept)) == [-3.0e38, 3.0e38]
        assert all(hc.stays_far(v, n, torch.float64) for v in hc.far_values(n))
    assert hc.overflow_case(c, hq, torch.float64) is None  # float64 arithmetic: every value of the list stays FAR
    far64 = hc.far_case(hc.plain_case("f64")[0], hc.plain_case("f64")[1], torch.float64)
    assert (np.abs(far64["loc"]) == 3.0e38).any()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pm,ac", MODES, ids=[mode_key(*m) for m in MODES])
def test_far_cases_oracles_are_finite_and_agree(oracle, name, pm, ac):
    c, hq, storage = hc.plain_case(name)
    if storage == torch.float64:
        # float64 arithmetic keeps the whole list (+-3.0e38 too): its oracle is finite there; the two oracles are held to
        # each other on the values that are FAR in float32 arithmetic as well
        full = run_oracle(oracle, hc.far_case(c, hq, storage), pm, ac, np.float64)
        assert all(np.isfinite(full[k]).all() for k in TENSORS)
        storage = F32
    far = hc.far_case(c, hq, storage)
    r32, r64 = run_oracle(oracle, far, pm, ac, np.float32), run_oracle(oracle, far, pm, ac, np.float64)
    keep = ~kink_mask(far["loc"], far["shapes"], ac)
    for k in TENSORS:
        assert np.isfinite(r32[k]).all() and np.isfinite(r64[k]).all(), k
        a, b = r32[k], r64[k]
        if k == "grad_loc":
            a, b = np.where(keep, a, 0), np.where(keep, b, 0)
        np.testing.assert_allclose(a, b, err_msg=k, **(FWD_TOL if k == "out" else BWD_TOL)[F32])
    # far samples: "zeros" drops them, "border" clips the location gradient
    hostile_far = np.abs(far["loc"][0][hq]) > 1e3
    assert hostile_far.any() and not r64["grad_loc"][0][hq][hostile_far].any()
    if far["value"].dtype == np.float32:
        np.testing.assert_allclose(native_forward(far, pm, ac), r32["out"], **FWD_TOL[F32])


@pytest.mark.parametrize("name", ["d32_vec_g8", "d5_scalar", "f64"])
@pytest.mark.parametrize("where", ["loc", "attn"])
@pytest.mark.parametrize("vname", list(hc.NONFINITE))
def test_nonfinite_input_is_contained_by_the_operation(oracle, name, where, vname):
    c, hq, _ = hc.plain_case(name)
    nf, planted = hc.nonfinite_case(c, hq, hc.NONFINITE[vname], where)
    clean = hc.check_plant(nf, c, hq)
    for pm, ac in MODES:
        for dtype in (np.float32, np.float64):
            got, want = run_oracle(oracle, nf, pm, ac, dtype), run_oracle(oracle, c, pm, ac, dtype)
            for k in ("out", "grad_loc", "grad_attn"):
                assert same_bits(got[k][1:], want[k][1:]) and same_bits(got[k][0][clean], want[k][0][clean]), (k, pm, ac)
            assert same_bits(got["grad_value"][1:], want["grad_value"][1:]), (pm, ac)
            if where == "loc" and pm == "zeros":  # item 4: such a sample contributes nothing to grad_value
                neutral = run_oracle(oracle, hc.neutralised(nf, planted), pm, ac, dtype)
                assert np.isfinite(got["grad_value"]).all()
                np.testing.assert_allclose(got["grad_value"], neutral["grad_value"], **BWD_TOL[torch.float32 if dtype == np.float32 else torch.float64])
        if c["value"].dtype == np.float32:
            got, want = native_forward(nf, pm, ac), native_forward(c, pm, ac)
            assert same_bits(got[1:], want[1:]) and same_bits(got[0][clean], want[0][clean]), ("native", pm, ac)


@pytest.mark.parametrize("name", ["d32_vec_g8", "d5_scalar"])
def test_a_pixel_coordinate_that_overflows_float32_is_contained_like_any_non_finite_one(oracle, name):
    """+-3.0e38: finite in float32, x * w is not.  The float32 oracle (as the reference's kernels) then forms inf - inf in
    the hostile rows and nowhere else; in float64 the same case is an ordinary far one."""
    c, hq, storage = hc.plain_case(name)
    over = hc.overflow_case(c, hq, storage)
    clean = hc.check_plant(over, c, hq)
    for pm, ac in MODES:
        got, want = run_oracle(oracle, over, pm, ac, np.float32), run_oracle(oracle, c, pm, ac, np.float32)
        for k in ("out", "grad_loc", "grad_attn"):
            assert same_bits(got[k][1:], want[k][1:]) and same_bits(got[k][0][clean], want[k][0][clean]), (k, pm, ac)
        assert same_bits(got["grad_value"][1:], want["grad_value"][1:]), (pm, ac)
        assert not np.isfinite(got["out"][0][hq]).all()  # (which is why it cannot be a FAR case in float32)
        r64 = run_oracle(oracle, over, pm, ac, np.float64)
        assert all(np.isfinite(r64[k]).all() for k in TENSORS)
        got, want = native_forward(over, pm, ac), native_forward(c, pm, ac)
        assert same_bits(got[1:], want[1:]) and same_bits(got[0][clean], want[0][clean]), ("native", pm, ac)


@pytest.mark.parametrize("where", ["offset", "logit", "ref"])
def test_fused_planting_touches_the_hostile_queries_only(where):
    g = torch.Generator().manual_seed(1)
    hq = hc.hostile_queries(40, 3)
    clean = np.ones(40, dtype=bool)
    clean[hq] = False
    for proj, ref in ((torch.randn(2, 40, 3, 4, 2, 3, generator=g), torch.rand(2, 40, 4, 2, generator=g)),
                      (torch.randn(2, 40, 3, 12, 3, generator=g), torch.rand(2, 40, 4, generator=g))):
        for values in (hc.fused_far_values(), [float("nan")], [float("inf"), float("-inf")]):
            p2, r2 = hc.plant_fused(proj, ref, hq, values, where)
            assert torch.equal(p2[1:], proj[1:]) and torch.equal(r2[1:], ref[1:])
            assert torch.equal(p2[0][clean], proj[0][clean]) and torch.equal(r2[0][clean], ref[0][clean])
            changed = (r2[0][hq] != ref[0][hq]) if where == "ref" else (p2[0][hq] != proj[0][hq])
            assert bool(changed.flatten(1).any(1).all())  # every hostile query got something
            if where == "ref":
                assert torch.equal(p2, proj) and torch.equal(r2[0][hq][..., 1:], ref[0][hq][..., 1:])
            else:
                ch = slice(2, 3) if where == "logit" else slice(0, 2)
                other = slice(0, 2) if where == "logit" else slice(2, 3)
                assert torch.equal(r2, ref) and torch.equal(p2[..., other], proj[..., other])
                assert bool((p2[0][hq][..., ch] == proj[0][hq][..., ch]).any())  # some samples stay benign
