"""GPU: every kernel family within the DERIVED rounding-error bound of tests/error_bound_cases.py on generic inputs —
|got - val| <= err * (1 + 2^-10) + r per element, val the fp64 value, err the first-order bound of a float evaluation with the
kernels' operations, r half the spacing of the type the result came back in (0 for float32: one rounding on store).  The
bound is 10 to 13 bits tighter than the smoke tolerances of tests/test_gpu_parity.py: a kernel that carries 16-bit bilinear
fractions, 16-bit corner weights, a 16-bit accumulator or a second rounding of a partial sum fails here
(tests/test_error_bound_cases.py shows each of those mutants outside the bound on these very fixtures).  Run with ``-m gpu``.

Every run prints its largest error / bound per tensor.  grad_value is compared with the formula of the route that ran, read
back from `last_launch_info`: the sorted pipeline's 20-bit record fractions or the single-launch kernel's float ones."""
import numpy as np
import pytest
import torch

import error_bound_cases as eb
from error_bound_cases import MODES, STORAGE
from test_gpu_exact_numerics import launch_info, options

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODE_IDS = [f"{pm}_{int(ac)}" for pm, ac in MODES]
NAN = float("nan")


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)


def run(c, pm, ac, storage, layout="dense", discrete=False, vmask=None, qmask=None):
    """The case through the public API (autograd -> C ABI -> HIP), as test_gpu_exact_numerics.run; the results on the CPU
    in the types they came back in.  vmask ([B, I] bool, True = real): padded pixels hold NaN; qmask ([B, Q] bool): padded
    queries' sampling points and weights hold NaN."""
    from msda_triton_amd import multiscale_deformable_attention
    from msda_triton_amd.functional import padded_value_rows
    vdt, cdt = STORAGE[storage]
    v = _dev(c["value"], vdt)
    loc, attn = _dev(c["loc"], cdt), _dev(c["attn"], cdt)
    kw = {}
    if vmask is not None:
        m = torch.from_numpy(vmask).to(DEV)
        v = torch.where(m[:, :, None, None], v, torch.full_like(v, NAN))
        kw["value_mask"] = m
    if qmask is not None:
        m = torch.from_numpy(qmask).to(DEV)
        loc = torch.where(m.reshape(m.shape + (1,) * (loc.dim() - 2)), loc, torch.full_like(loc, NAN))
        attn = torch.where(m.reshape(m.shape + (1,) * (attn.dim() - 2)), attn, torch.full_like(attn, NAN))
        kw["query_mask"] = m
    if layout == "padded":
        vp = padded_value_rows(*v.shape, v.dtype, v.device, pad_bytes=128)
        vp.copy_(v)
        v = vp
        assert not v.is_contiguous()
    v.requires_grad_(True)
    loc.requires_grad_(not discrete)
    attn.requires_grad_(True)
    if "counts" in c:
        kw["points_per_level"] = c["counts"]
    if discrete:
        kw["sampling_mode"] = "discrete"
    out = multiscale_deformable_attention(v, torch.from_numpy(np.array(c["shapes"])).to(DEV), loc, attn, pm, ac, **kw)
    out.backward(_dev(c["grad_out"], cdt))
    torch.cuda.synchronize()
    assert out.dtype == cdt and v.grad.dtype == vdt and attn.grad.dtype == cdt
    got = dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_attn=attn.grad.cpu())
    if not discrete:
        got["grad_loc"] = loc.grad.cpu()
    return got


def check(name, pm, ac, storage, route=None, **kw):
    """One run of the plain operator against the formulas of the grad_value route that ran (route: the one expected)."""
    got = run(eb.get_case(name, storage), pm, ac, storage, **kw)
    info = launch_info()
    assert info["value_path"] in (1, 2), info
    if route is not None:
        assert info["value_path"] == route, info
    form, keep = eb.plain_reference(name, storage, pm, ac, "q20" if info["value_path"] == 2 else "float")
    eb.assert_within(got, form, keep, f"{name} {pm} {int(ac)} {storage} value_path={info['value_path']} {kw or ''}")
    return info


# ----------------------------------------------------------------------------------------- modes x storage x head dimension
@pytest.mark.parametrize("storage", list(STORAGE))
@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["d32", "d5", "d64"])
def test_plain_operator_default_route(name, pm, ac, storage):
    check(name, pm, ac, storage)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("value_path", [2, 3], ids=["sorted_gather", "single_launch"])
@pytest.mark.parametrize("name", ["d32", "d5", "d64", "counts"])
def test_both_grad_value_routes(name, value_path, storage):
    with options(value_path=value_path):
        for pm, ac in MODES:
            check(name, pm, ac, storage, route=2 if value_path == 2 else 1)


# ----------------------------------------------------------------------------------------- long sums, wide range
LONG_ROUTES = {
    "single_launch": (dict(value_path=3), 1),
    "sorted_gather": (dict(value_path=2), 2),
    "sorted_rounds": (dict(value_path=2, q_round=64), 2),
    "sorted_passes": (dict(value_path=2, ws_passes=2), 2),
}


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("route", list(LONG_ROUTES))
def test_long_grad_value_sums(route, storage):
    """Hundreds of terms per grad_value element: across gather workgroups, rounds of queries and passes over the batch."""
    opts, path = LONG_ROUTES[route]
    with options(**opts):
        for pm, ac in MODES:
            info = check("long_sum", pm, ac, storage, route=path)
            if "ws_passes" in opts:
                assert info["value_passes"] == 2, info


@pytest.mark.parametrize("name,storage", [("range", "f32"), ("range", "bf16"), ("range", "f32_vbf16"), ("range_h", "fp16"),
                                          ("range_h", "f32_vf16")])
@pytest.mark.parametrize("value_path", [2, 3], ids=["sorted_gather", "single_launch"])
def test_wide_range_with_cancellation(name, storage, value_path):
    with options(value_path=value_path):
        for pm, ac in MODES:
            check(name, pm, ac, storage, route=2 if value_path == 2 else 1)


# ----------------------------------------------------------------------------------------- forced kernel variants
@pytest.mark.parametrize("storage", ["f32", "f32_vbf16"])
def test_lds_served_levels(storage):
    with options(unit_fwd=0, lds_levels=2):
        for pm, ac in MODES:
            info = check("long_sum", pm, ac, storage)
            assert info["fwd_variant"] == 1 and info["sample_variant"] == 1, info


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_one_wave_per_unit_forward(storage):
    with options(unit_fwd=2):
        for pm, ac in MODES:
            assert check("d32", pm, ac, storage)["fwd_variant"] == 2


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_padded_value_rows(storage):
    for pm, ac in MODES:
        check("d32", pm, ac, storage, layout="padded")


# ----------------------------------------------------------------------------------------- the mask twins
def _masks(name):
    c = eb.raw_case(name)
    rng = np.random.default_rng(11)
    vmask = rng.random(c["value"].shape[:2]) > 0.25
    qmask = rng.random(c["grad_out"].shape[:2]) > 0.25
    return vmask, qmask


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["value_mask", "query_mask"])
def test_mask_twins_against_the_pre_masked_problem(which, storage):
    """Padded pixels / padded queries hold NaN; the reference is the problem with them zeroed beforehand."""
    vmask, qmask = _masks("d32")
    vmask, qmask = (vmask, None) if which == "value_mask" else (None, qmask)
    c = eb.get_case("d32", storage)
    pre = eb.masked_case(c, vmask, qmask)
    for pm, ac in MODES:
        got = run(c, pm, ac, storage, vmask=vmask, qmask=qmask)
        info = launch_info()
        form = eb.plain_formulas(pre, pm, ac, "q20" if info["value_path"] == 2 else "float")
        if vmask is not None:  # a padded pixel's grad_value row is stored as zeros
            gv = form["grad_value"]
            form["grad_value"] = gv.where(vmask[:, :, None, None])
        eb.assert_within(got, form, eb.plain_keep(pre, ac), f"d32 {which} {pm} {int(ac)} {storage}")


# ----------------------------------------------------------------------------------------- discrete sampling
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("value_path,route", [(3, 1), (2, 2)], ids=["single_launch", "sorted_gather"])
def test_discrete_sampling(value_path, route, storage):
    form, keep, _ = eb.discrete_reference("discrete", storage)
    with options(value_path=value_path):
        got = run(eb.get_case("discrete", storage), "border", False, storage, discrete=True)
        info = launch_info()
    assert info["fwd_variant"] == 3 and info["sample_variant"] == 2 and info["value_path"] == route, info
    eb.assert_within(got, form, keep, f"discrete {storage} value_path={value_path}")


# ----------------------------------------------------------------------------------------- the fused families
FUSED_KERNELS = {"module2": "fused", "module4": "fused", "module2_c": "fused_ragged", "module4_c": "fused_ragged",
                 "levelref2": "fused_levelref", "levelref4": "fused_levelref", "hfbox": "fused_hfbox",
                 "hfbox_discrete": "fused_hfbox_discrete"}


def run_fused(name, fc, pm, ac, storage, vmask=None, qmask=None):
    """The family's public entry point under a KernelTimer (so the Python Function launches and names its kernels);
    asserts that the fused pair ran and no other forward.  Masks as in `run`: padded pixels, and padded queries' projection
    and reference-point rows, hold NaN."""
    from msda_triton_amd.functional import KernelTimer, fused_hf_box_core, fused_hf_module_core, fused_module_core
    sdt, rdt = eb.FUSED_STORAGE[storage]
    rule, _, _ = eb.FUSED[name]
    v, pr, rf = _dev(fc["value"], sdt), _dev(fc["proj"], sdt), _dev(fc["ref"], rdt)
    kw = {}
    if vmask is not None:
        m = torch.from_numpy(vmask).to(DEV)
        v = torch.where(m[:, :, None, None], v, torch.full_like(v, NAN))
        kw["value_mask"] = m
    if qmask is not None:
        m = torch.from_numpy(qmask).to(DEV)
        pr = torch.where(m.reshape(m.shape + (1,) * (pr.dim() - 2)), pr, torch.full_like(pr, NAN))
        rf = torch.where(m.reshape(m.shape + (1,) * (rf.dim() - 2)), rf, torch.full_like(rf, NAN))
        kw["query_mask"] = m
    discrete = name == "hfbox_discrete"
    v.requires_grad_(True)
    pr.requires_grad_(True)
    rf.requires_grad_(not discrete)
    shapes = torch.from_numpy(np.array(fc["shapes"])).to(DEV)
    with KernelTimer() as kt:
        if rule == "hfbox":
            out = fused_hf_box_core(v, shapes, pr, rf, fc["counts"], eb.HFBOX_SCALE, *(() if discrete else (pm, ac)),
                                    sampling_mode="discrete" if discrete else "bilinear", **kw)
        elif rule == "levelref":
            out = fused_hf_module_core(v, shapes, pr, rf, pm, ac, **kw)
        else:
            out = fused_module_core(v, shapes, pr, rf, pm, ac, points_per_level=fc.get("counts"), **kw)
        out.backward(_dev(fc["grad_out"], sdt))
        torch.cuda.synchronize()
    launched = [r[0] for r in kt.records]
    fam = FUSED_KERNELS[name]
    assert [n for n in launched if n.startswith("msda_fwd")] == [f"msda_fwd_{fam}"] and f"msda_bwd_{fam}" in launched, launched
    assert out.dtype == sdt and v.grad.dtype == sdt and pr.grad.dtype == sdt
    got = dict(out=out.detach().cpu(), grad_value=v.grad.cpu(), grad_proj=pr.grad.cpu())
    if not discrete:
        assert rf.grad.dtype == rdt
        got["grad_ref"] = rf.grad.cpu()
    return got


def check_fused(name, pm, ac, storage="f32", route=None):
    got = run_fused(name, eb.fused_case(name, storage), pm, ac, storage)
    info = launch_info()
    assert info["value_path"] in (1, 2), info
    if route is not None:
        assert info["value_path"] == route, info
    form, keep, _ = eb.fused_reference(name, storage, pm, ac, "q20" if info["value_path"] == 2 else "float")
    eb.assert_within(got, form, keep, f"{name} {pm} {int(ac)} {storage} value_path={info['value_path']}")


BILINEAR_FUSED = [n for n in eb.FUSED if n != "hfbox_discrete"]


@pytest.mark.parametrize("pm,ac", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", BILINEAR_FUSED)
def test_fused_families_f32(name, pm, ac):
    check_fused(name, pm, ac)


@pytest.mark.parametrize("value_path", [2, 3], ids=["sorted_gather", "single_launch"])
@pytest.mark.parametrize("name", BILINEAR_FUSED + ["hfbox_discrete"])
def test_fused_families_both_grad_value_routes(name, value_path):
    with options(value_path=value_path):
        check_fused(name, "zeros", False, route=2 if value_path == 2 else 1)


@pytest.mark.parametrize("storage,pm,ac", [("f32_sbf16", "zeros", False), ("f32_sf16", "border", True)], ids=["sbf16", "sf16"])
@pytest.mark.parametrize("name", BILINEAR_FUSED + ["hfbox_discrete"])
def test_fused_families_16_bit_storage(name, storage, pm, ac):
    check_fused(name, pm, ac, storage)


@pytest.mark.parametrize("name", ["module4", "module4_c"], ids=["fused_masked", "fused_ragged_masked"])
def test_module_masked_pair_against_the_pre_masked_problem(name):
    from test_gpu_module_masks import spied_symbols
    fc = eb.fused_case(name)
    rng = np.random.default_rng(12)
    vmask = rng.random(fc["value"].shape[:2]) > 0.25
    qmask = rng.random(fc["grad_out"].shape[:2]) > 0.25
    pre = dict(fc, value=np.where(vmask[:, :, None, None], fc["value"], 0.0),
               grad_out=np.where(qmask[:, :, None, None], fc["grad_out"], 0.0))
    log = []
    with spied_symbols(log):
        got = run_fused(name, fc, "zeros", False, "f32", vmask=vmask, qmask=qmask)
    fam = FUSED_KERNELS[name]
    assert log == [f"msda_fwd_{fam}_masked_f32", f"msda_bwd_{fam}_masked_f32"], log
    info = launch_info()
    form, keep, _ = eb.fused_formulas(pre, name, "zeros", False, "q20" if info["value_path"] == 2 else "float")
    form["out"] = form["out"].where(qmask[:, :, None, None])                 # a padded query's row of `out` is zeros
    form["grad_value"] = form["grad_value"].where(vmask[:, :, None, None])    # a padded pixel's grad_value row is zeros
    eb.assert_within(got, form, keep, f"{name} masked")
