"""DESIGN.md §5 held with NO tolerance: on the exactly representable inputs of tests/exact_cases.py every correct
float32 / float64 evaluation of the operator is exact in any order, so the kernels' results must EQUAL the fp64 CPU
oracle bit for bit in f32 and f64, and that reference rounded to nearest even ONCE in fp16 / bf16 (and, with mixed
storage, in whatever type each tensor comes back in) — out, grad_value, grad_loc and grad_attn, no mask.  A kernel
that accumulates in 16 bits, truncates on store, rounds a partial sum between rounds / passes / workgroups, carries
coarser weights than documented or drops a small corner fails here (tests/test_exact_cases.py shows each of those
mutants differs from `expected` on these very fixtures).  Run with ``-m gpu``.

Every comparison below is an equality; the precondition (budget <= 24 bits, float32 oracle == float64 oracle) is
asserted by `checked_reference` before the GPU is touched."""
import contextlib

import numpy as np
import pytest
import torch

import exact_cases as ec
from exact_cases import BF16, F16, F32, F64, MODES, TENSORS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODE_IDS = [f"{pm}_{int(ac)}" for pm, ac in MODES]
# name: (value / grad_value storage, storage of everything else)
STORAGE = {"f32": (F32, F32), "f64": (F64, F64), "fp16": (F16, F16), "bf16": (BF16, BF16), "f32_vbf16": (BF16, F32),
           "f32_vf16": (F16, F32)}


@contextlib.contextmanager
def options(**kw):
    from msda_triton_amd import _lib
    old = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def launch_info():
    from msda_triton_amd import _lib
    return _lib.last_launch_info()


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)


def run(c, pm, ac, vdt, cdt, layout="dense", discrete=False, mask=None):
    """The case through the public API (autograd -> C ABI -> HIP) the way test_gpu_parity.run_hip goes; the results
    on the CPU in the types they came back in.  `mask` ([B, I] bool on the host, True = real pixel): the value-mask twins,
    on a pyramid whose padding pixels hold NaN."""
    from msda_triton_amd import multiscale_deformable_attention
    from msda_triton_amd.functional import padded_value_rows
    v = _dev(c["value"], vdt)
    if mask is not None:
        v = torch.where(mask.to(DEV)[:, :, None, None], v, torch.full_like(v, float("nan")))
    if layout == "padded":
        vp = padded_value_rows(*v.shape, v.dtype, v.device, pad_bytes=128)
        vp.copy_(v)
        v = vp
        assert not v.is_contiguous()
    elif layout == "unaligned":  # contiguous, but its rows start only 4 bytes into a 16-byte unit: the scalar path
        off = 4 // v.element_size()
        flat = torch.zeros(v.numel() + off, dtype=vdt, device=DEV)
        flat[off:] = v.reshape(-1)
        v = flat[off:].reshape(v.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    v.requires_grad_(True)
    loc = _dev(c["loc"], cdt).requires_grad_(not discrete)
    attn = _dev(c["attn"], cdt).requires_grad_(True)
    kw = dict(points_per_level=c["counts"]) if "counts" in c else {}
    if discrete:
        kw["sampling_mode"] = "discrete"
    if mask is not None:
        kw["value_mask"] = mask.to(DEV)
    out = multiscale_deformable_attention(v, torch.from_numpy(np.array(c["shapes"])).to(DEV), loc, attn, pm, ac, **kw)
    out.backward(_dev(c["grad_out"], cdt))
    torch.cuda.synchronize()
    assert out.dtype == cdt and v.grad.dtype == vdt and attn.grad.dtype == cdt
    got = dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_attn=attn.grad.cpu())
    if not discrete:
        assert loc.grad.dtype == cdt
        got["grad_loc"] = loc.grad.cpu()
    return got


def assert_exact(got, ref, what):
    """Every tensor equals the reference rounded once to the type it came back in.  All four are compared before the
    assertion so that a failure names every tensor that is off."""
    wrong = {}
    for k, r in ref.items():
        want = ec.expected(r, got[k].dtype)
        assert got[k].shape == want.shape, (what, k)
        if not torch.equal(got[k], want):
            ne = got[k] != want
            wrong[k] = (int(ne.sum()), float((got[k].double() - want.double()).abs().max()))
    print(f"{what}: " + (f"NOT exact: {wrong} (elements off, largest difference)" if wrong else "exact"))
    assert not wrong, (what, wrong)


def check(name, pm, ac, storage, layout="dense"):
    vdt, cdt = STORAGE[storage]
    ref = ec.checked_reference(name, pm, ac)
    assert set(ref) == set(TENSORS)
    assert_exact(run(ec.get_case(name), pm, ac, vdt, cdt, layout), ref, f"{name} {pm} {int(ac)} {storage} {layout}")


# ----------------------------------------------------------------------------------------- shapes x modes x storage
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ec.SHAPE_MATRIX)
def test_shape_matrix_is_exact(name, pm, ac, storage):
    check(name, pm, ac, storage)


# ----------------------------------------------------------------------------------------- forced kernel variants
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("value_path", [2, 3], ids=["sorted_gather", "single_launch"])
@pytest.mark.parametrize("name", ["d32_vec_g8", "d5_scalar"])
def test_both_grad_value_paths_are_exact(name, value_path, storage):
    with options(value_path=value_path):
        for pm, ac in MODES:
            check(name, pm, ac, storage)
            assert launch_info()["value_path"] == (2 if value_path == 2 else 1)


# (float arithmetic on 16-byte pieces: f32, and 16-bit rows next to f32 sampling inputs; pure bf16 storage has no LDS variant)
@pytest.mark.parametrize("storage", ["f32", "f32_vbf16"])
@pytest.mark.parametrize("planes", [1, 2], ids=["one_plane", "two_planes"])
def test_lds_served_levels_are_exact(planes, storage):
    with options(unit_fwd=0, lds_levels=2, lds_planes=planes):
        for pm, ac in MODES:
            check("lds_q200", pm, ac, storage)
            info = launch_info()
            assert info["fwd_variant"] == 1 and info["fwd_lds_planes"] == planes and info["sample_variant"] == 1, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["d32_vec_g8", "lds_q200"])
def test_one_wave_per_unit_forward_is_exact(name, storage):
    with options(unit_fwd=2):
        for pm, ac in MODES:
            check(name, pm, ac, storage)
            assert launch_info()["fwd_variant"] == 2


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("q_round", [7, 20])
def test_sorted_pipeline_in_rounds_of_queries_is_exact(q_round, storage):
    with options(value_path=2, q_round=q_round):
        for pm, ac in MODES:
            check("d32_vec_g8", pm, ac, storage)
            assert launch_info()["value_path"] == 2


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("passes", [2, 4])
def test_passes_over_the_batch_are_exact(passes, storage):
    with options(value_path=2, ws_passes=passes):
        for pm, ac in MODES:
            check("b4_passes", pm, ac, storage)
            info = launch_info()
            assert info["value_path"] == 2 and info["value_passes"] == passes


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["d32_vec_g8", "d64_vec_g16"])
def test_padded_value_rows_are_exact(name, storage):
    for pm, ac in MODES:
        check(name, pm, ac, storage, layout="padded")


@pytest.mark.parametrize("storage", ["f32", "f32_vbf16", "bf16"])
def test_four_byte_aligned_view_is_exact(storage):
    """Rows that start 4 bytes into a 16-byte unit take the scalar kernels.  Which kernels ran is read off the launcher:
    with the LDS-served levels forced, a dense f32 / f32_vbf16 call takes them (they exist for 16-byte pieces only) and
    the same call on the view does not."""
    with options(unit_fwd=0, lds_levels=2):
        for pm, ac in MODES:
            if storage != "bf16":
                check("unaligned", pm, ac, storage)
                assert launch_info()["fwd_variant"] == 1
            check("unaligned", pm, ac, storage, layout="unaligned")
            assert launch_info()["fwd_variant"] == 0


# ----------------------------------------------------------------------------------------- thousands of samples in one cell
FLOOD_ROUTES = {
    "single_launch": dict(value_path=3),
    "sorted_gather": dict(value_path=2),
    "sorted_rounds_and_passes": dict(value_path=2, q_round=64, ws_passes=2),
}


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("route", list(FLOOD_ROUTES))
def test_flooded_cell_is_exact(route, storage):
    """2 048 samples per (plane, level) in ONE bilinear cell: its four pixels' grad_value rows are sums that the sorted
    pipeline splits over work items, gather workgroups, rounds of queries and passes over the batch, and the
    single-launch kernel over lane groups — exact partial sums, so any rounding on the way shows."""
    with options(**FLOOD_ROUTES[route]):
        for pm, ac in MODES:
            check("flood", pm, ac, storage)
            assert launch_info()["value_path"] == (1 if route == "single_launch" else 2)


# ----------------------------------------------------------------------------------------- per-level point counts
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("value_path", [0, 2, 3])
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["ragged_363", "ragged_125"])
def test_points_per_level_is_exact(name, pm, ac, value_path, storage):
    with options(value_path=value_path):
        check(name, pm, ac, storage)
        if value_path:
            assert launch_info()["value_path"] == (2 if value_path == 2 else 1)


# ----------------------------------------------------------------------------------------- discrete sampling
@pytest.mark.parametrize("storage", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name,value_path,route", [("discrete_363", 3, 1), ("discrete_363", 2, 2), ("discrete_sorted", 0, 2)],
                         ids=["single_launch", "sorted_forced", "sorted_by_size"])
def test_discrete_sampling_is_exact(name, value_path, route, storage):
    """out, grad_value and grad_attn against test_discrete_sampling.ref_discrete (fp64), on both grad_value routes."""
    vdt, cdt = STORAGE[storage]
    ref = ec.checked_reference(name)
    with options(value_path=value_path):
        got = run(ec.get_case(name), "border", False, vdt, cdt, discrete=True)
        info = launch_info()
    assert_exact(got, ref, f"{name} {storage} value_path={value_path}")
    assert info["fwd_variant"] == 3 and info["sample_variant"] == 2 and info["value_path"] == route
