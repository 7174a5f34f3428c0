"""Deformable feature aggregation on the GPU: msda_dfa_{fwd,bwd}_<dtype> through the public function against the float64
index-arithmetic reference on the CPU (dfa_cases.py) — every element of out and the three gradients.  ONE test id on
purpose: the topics below run one after another inside it (a few seconds in all), and a failure names its topic and case."""
import pytest
import torch

import dfa_cases as fc
from test_gpu_parity import BWD_TOL, FWD_TOL
from test_ragged_points import TOL as TOL16

pytestmark = pytest.mark.gpu
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16


def tolerances(dtype):
    if dtype in FWD_TOL:
        return FWD_TOL[dtype], BWD_TOL[dtype]
    atol, rtol = TOL16[dtype]
    return dict(atol=atol, rtol=rtol), dict(atol=atol, rtol=rtol)


def gpu_run(shapes, inputs, dtype, **kw):
    from msda_triton_amd import deformable_aggregation
    return fc.run(deformable_aggregation, shapes, inputs, dtype, "cuda", **kw)


def check(dtype=F64, seed=0, value_path=1, **over):
    from msda_triton_amd import _lib
    shapes, inputs, want = fc.case(dtype, seed, **over)
    got = gpu_run(shapes, inputs, dtype)
    info = _lib.last_launch_info()
    assert (info["fwd_variant"], info["sample_variant"], info["value_path"]) == (7, 6, value_path), info
    fc.assert_close(got, want, *tolerances(dtype), label=f"{dtype} {over}: ")
    return info


# C = 8; C = 32: the 16-byte path; G 2 x D 36: one element per lane in 16 bits, where group 1 also straddles two chunks;
# C = 256, G = 8: a full wave per unit (two chunks in fp64); and the first row of 16-byte pieces beyond one wave's chunk
def base_case_storage_types_and_row_widths(dtype):
    size = torch.empty((), dtype=dtype).element_size()
    vec = 16 // size
    for G, D in [(2, 4), (2, 16), (2, 36), (8, 32), (2, 33 * vec)]:
        info = check(dtype, G=G, D=D)
        want_vec = vec if (D * size) % 16 == 0 else 1
        want_chunks = -(-G * D // (64 * want_vec))
        assert info["fwd_vec"] == info["sample_vec"] == want_vec, (dtype, G, D, info)
        assert info["fwd_chunks"] == info["sample_chunks"] == want_chunks and (D != 33 * vec or want_chunks == 2), (dtype, G, D, info)


# more records than one trip holds, at 16 units per wave and at one; A * P > 4096 samples per plane and level (the
# route's threshold): grad_feature_maps through the sorted pipeline (every other case here takes the single-launch kernel)
def trips_and_the_sorted_pipeline():
    from msda_triton_amd import _lib
    lib = _lib.load()
    for dtype, over in [(F32, dict(P=7)), (BF16, dict(P=7)), (F32, dict(B=1, A=3, P=50, G=8, D=32)), (F64, dict(P=9, G=3, D=6))]:
        size = torch.empty((), dtype=dtype).element_size()
        G, D, P = over.get("G", 2), over.get("D", 4), over["P"]
        for bwd in (0, 1):
            cap = lib.msda_dfa_trip_records(G * D, G, 3, 2, size, bwd)
            assert 0 < cap < P * 6 and cap % 6 == 0, (dtype, over, bwd, cap)
        info = check(dtype, seed=1, **over)
        assert info["fwd_trips"] == -(-P * 6 // lib.msda_dfa_trip_records(G * D, G, 3, 2, size, 0)) >= 2, info
        assert info["sample_trips"] == -(-P * 6 // lib.msda_dfa_trip_records(G * D, G, 3, 2, size, 1)) >= 2, info
    for dtype in (F32, BF16):
        check(dtype, seed=2, value_path=2, B=1, A=230, P=18, G=2, D=16)


POW2 = (((4, 8), (2, 4)), ((8, 4), (4, 2)))


def reruns_frozen_maps_and_exact_inputs_are_bitwise():
    from msda_triton_amd import _lib
    shapes, inputs, _ = fc.case(F32, G=8, D=32)
    first, again = gpu_run(shapes, inputs, F32), gpu_run(shapes, inputs, F32)
    frozen = gpu_run(shapes, inputs, F32, needs=(False, True, True))
    assert frozen["grad_feature_maps"] is None and _lib.last_launch_info()["sample_variant"] == 6
    for name in fc.NAMES:
        assert torch.equal(again[name], first[name]), name
        assert name == "grad_feature_maps" or torch.equal(frozen[name], first[name]), name
    for dtype in (F32, F64):  # small integers on power-of-two maps at pixel centres, weights of ones: no rounding anywhere
        shapes, inputs, want = fc.case(dtype, 3, exact=True, shapes=POW2, G=2, D=16)
        got = gpu_run(shapes, inputs, dtype)
        assert _lib.last_launch_info()["fwd_variant"] == 7
        for name in fc.NAMES:
            assert torch.equal(got[name], want[name]), (dtype, name)


def more_than_32_maps_take_the_composition():
    shapes33 = tuple(((3, 4), (2, 3), (2, 2)) for _ in range(11))
    shapes, inputs, want = fc.case(F64, 4, shapes=shapes33, A=3, P=2)
    fc.assert_close(gpu_run(shapes, inputs, F64), want, FWD_TOL[F64], BWD_TOL[F64])


def test_deformable_aggregation_kernels():
    for dtype in (F64, F32, BF16, F16):
        base_case_storage_types_and_row_widths(dtype)
    trips_and_the_sorted_pipeline()
    reruns_frozen_maps_and_exact_inputs_are_bitwise()
    more_than_32_maps_take_the_composition()
