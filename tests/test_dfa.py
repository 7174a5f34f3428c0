"""Deformable feature aggregation on host tensors: the PyTorch formulation and the expansion into
multiscale_deformable_attention against the float64 index-arithmetic reference (dfa_cases.py), and the public function's
argument errors."""
import pytest
import torch

import dfa_cases as fc
from msda_triton_amd import deformable_aggregation, native_deformable_aggregation

TOL = dict(atol=1e-9, rtol=1e-9)


@pytest.mark.parametrize("fn", [deformable_aggregation, native_deformable_aggregation, fc.expansion], ids=lambda f: f.__name__)
@pytest.mark.parametrize("over", [dict(), dict(G=3, D=5, P=4)], ids=["base", "G3-D5-P4"])
def test_host_formulations_match_the_reference(fn, over):
    shapes, inputs, want = fc.case(**over)
    fc.assert_close(fc.run(fn, shapes, inputs), want, TOL, TOL)


def test_flat_feature_maps_and_float32():
    shapes, inputs, want = fc.case(torch.float32)
    flat = lambda fm, s, loc, w: deformable_aggregation(fm.flatten(2), s, loc, w).unflatten(2, (w.shape[-1], -1))  # noqa: E731
    got = fc.run(flat, shapes, inputs, torch.float32)
    fc.assert_close(got, want, dict(atol=1e-4, rtol=1e-3), dict(atol=1e-3, rtol=1e-2))


def test_argument_errors():
    shapes, inputs, _ = fc.case()
    fm, loc, wts = inputs["fm"], inputs["loc"], inputs["wts"]
    for bad in [(fm, shapes[:2], loc, wts), (fm, shapes.double(), loc, wts), (fm, shapes, loc[:, :, :, :2], wts),
                (fm, shapes, loc, wts[..., 0]), (fm.flatten(2)[..., :7], shapes, loc, wts), (fm[:, :, :1], shapes, loc, wts),
                (fm.float(), shapes, loc, wts), (fm[:, :-1], shapes, loc, wts)]:
        with pytest.raises(ValueError):
            deformable_aggregation(*bad)
