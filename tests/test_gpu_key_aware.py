"""Key-aware deformable attention on the GPU: msda_keyaware_{fwd,bwd}_<dtype> through the public function against the
float64 reference on the CPU (key_aware_cases.py) — every element of out, attn and the four gradients."""
import pytest
import torch

import key_aware_cases as kc
from test_gpu_parity import BWD_TOL, FWD_TOL
from test_ragged_points import TOL as TOL16

pytestmark = pytest.mark.gpu
F32 = torch.float32


def tolerances(dtype):
    if dtype in FWD_TOL:
        return FWD_TOL[dtype], BWD_TOL[dtype]
    atol, rtol = TOL16[dtype]
    return dict(atol=atol, rtol=rtol), dict(atol=atol, rtol=rtol)


def gpu_run(inputs, levels, pm="border", ac=False, dtype=F32, **kw):
    from msda_triton_amd import key_aware_deformable_attention
    return kc.run(key_aware_deformable_attention, inputs, levels, pm, ac, dtype, "cuda", **kw)


def check(pm="border", ac=False, dtype=F32, **shape):
    inputs, want = kc.case(dtype=dtype, pm=pm, ac=ac, **shape)
    got = gpu_run(inputs, shape.get("levels", kc.BASE_LEVELS), pm, ac, dtype)
    kc.assert_close(got, want, *tolerances(dtype))
    return got


def launch_info():
    from msda_triton_amd import _lib
    return _lib.last_launch_info()


# the base case in all four modes; then the head dimension away from it: one lane per unit, and a unit with idle lanes
@pytest.mark.parametrize("pm,ac,D", [(pm, ac, 32) for pm, ac in kc.MODES] + [("border", False, 4), ("border", False, 36)])
def test_base_case_every_mode_and_head_dim(pm, ac, D):
    check(pm, ac, D=D)
    info = launch_info()
    assert (info["fwd_variant"], info["fwd_group"], info["fwd_trips"]) == (5, {4: 4, 32: 8, 36: 16}[D], 1)
    assert info["value_path"] == 1  # (Q * P <= 4096: both pyramid gradients from the single-launch kernel)


# (bf16 with D = 36, no multiple of 16 bytes: the scalar path, VEC = 1 with 64-lane units)
@pytest.mark.parametrize("dtype,D", [(torch.float64, 32), (torch.bfloat16, 32), (torch.float16, 32), (torch.bfloat16, 36)])
def test_storage_types(dtype, D):
    check(dtype=dtype, D=D)
    assert launch_info()["fwd_vec"] == (16 // torch.empty((), dtype=dtype).element_size() if D == 32 else 1)


def test_one_sample_per_unit():
    got = check(levels=((4, 4),), P=1, seed=1)
    assert torch.equal(got["attn"], torch.ones_like(got["attn"]))


def test_sixteen_samples():
    check(levels=((5, 7), (3, 2), (1, 1), (2, 3)), P=4, seed=2)


def test_softmax_state_crosses_a_trip():
    """One sample more than the forward parks per trip; the query times 8 and the largest key under the unit's last sample,
    so that the running maximum moves in the last trip and the first trip's attention rows are rescaled."""
    from msda_triton_amd import _lib
    P = int(_lib.load().msda_keyaware_trip_samples(32, 4)) + 1
    check("zeros", levels=((5, 7),), P=P, Q=21, seed=4, peaked=True)
    info = launch_info()
    assert info["fwd_trips"] == 2 and info["sample_trips"] >= 2


def test_both_pyramid_gradients_through_the_sorted_pipeline():
    check(Q=1100, P=4, seed=5)
    assert launch_info()["value_path"] == 2


@pytest.mark.parametrize("frozen", ["key", "value", "both"])
def test_frozen_pyramids_leave_the_other_gradients_bitwise(frozen):
    inputs, _ = kc.case()
    full = gpu_run(inputs, kc.BASE_LEVELS)
    part = gpu_run(inputs, kc.BASE_LEVELS, needs=(True, frozen == "value", frozen == "key", True))
    for name in kc.NAMES:
        if part[name] is None:
            assert name == "grad_key" and frozen != "value" or name == "grad_value" and frozen != "key"
        else:
            assert torch.equal(part[name], full[name]), name


def test_padded_rows_and_a_second_run_are_bitwise():
    from msda_triton_amd.functional import padded_value_rows
    inputs, _ = kc.case()
    dense = gpu_run(inputs, kc.BASE_LEVELS)
    again = gpu_run(inputs, kc.BASE_LEVELS)
    pyramids = []
    for name in ("key", "value"):
        src = inputs[name].float().cuda()
        padded = padded_value_rows(*src.shape, F32, "cuda", pad_bytes=128)
        padded.copy_(src)
        assert not padded.is_contiguous()
        pyramids.append(padded)
    strided = gpu_run(inputs, kc.BASE_LEVELS, pyramids=pyramids)
    for name in kc.NAMES:
        assert torch.equal(again[name], dense[name]), name
        assert torch.equal(strided[name], dense[name]), name
