"""The head dimension D swept through every kernel family and storage type: D decides the template instantiation a call
runs (VEC channels per lane, G lanes per unit, channel chunks — tests/head_dim_cases.py), and the rest of the suite runs
almost everything at G <= 16 and one chunk.  Here every (VEC, G, chunks) class — G = 32 and 64 on the 16-byte and the
scalar path, two and more chunks, a partly filled group or last chunk, G = 16 for 16-bit rows — runs through the plain
pair, per-level counts, discrete sampling, the value-mask twins, both grad_value routes and the forced variants, on the
exact inputs of tests/exact_cases.py: every comparison is an EQUALITY with the fp64 oracle (rounded once for 16-bit
results).  `msda_last_launch_info` names the instantiation that ran, so a changed threshold cannot quietly turn a G = 64
test into a G = 16 one.  Run with ``-m gpu``."""
import pytest
import torch

import exact_cases as ec
import head_dim_cases as hd
from exact_cases import MODES
from test_gpu_exact_numerics import STORAGE, assert_exact, launch_info, options, run
from test_gpu_value_mask import make_mask

pytestmark = pytest.mark.gpu

ROUTES = {"sorted_gather": (2, 2), "single_launch": (3, 1)}  # name: (option value_path, launch info value_path)


def check(name, storage, want, what, families=("fwd", "sample", "value"), **run_kw):
    """The case in every mode: exact, and run by the instantiation `want` names."""
    vdt, cdt = STORAGE[storage]
    discrete = ec.CASES[name][0] == "discrete"
    for pm, ac in (MODES if not discrete else [("border", False)]):
        ref = ec.checked_reference(name, pm, ac) if not discrete else ec.checked_reference(name)
        got = run(ec.get_case(name), pm, ac, vdt, cdt, discrete=discrete, **run_kw)
        info = launch_info()
        assert_exact(got, ref, f"{what} {pm} {int(ac)}")
        hd.assert_info(info, want, what, families)
    return info


# ----------------------------------------------------------------------------------------- plain pair, per-level counts
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("storage", hd.STORAGES)
@pytest.mark.parametrize("kind", ["p3", "c25"])
@pytest.mark.parametrize("D", hd.HEAD_DIMS)
def test_bilinear_is_exact_in_the_expected_instantiation(D, kind, storage, route):
    opt, path = ROUTES[route]
    with options(value_path=opt):
        info = check(hd.case_name(D, kind), storage, hd.expect_info(storage, D), f"hd{D}_{kind} {storage} {route}")
    assert info["value_path"] == path and info["fwd_variant"] == 0 and info["sample_variant"] == 0, info


# ----------------------------------------------------------------------------------------- discrete sampling
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("storage", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("D", hd.HEAD_DIMS)
def test_discrete_is_exact_in_the_expected_instantiation(D, storage, route):
    opt, path = ROUTES[route]
    with options(value_path=opt):
        info = check(hd.case_name(D, "disc"), storage, hd.expect_info(storage, D), f"hd{D}_disc {storage} {route}")
    assert info["value_path"] == path and info["fwd_variant"] == 3 and info["sample_variant"] == 2, info


# ----------------------------------------------------------------------------------------- value-mask twins
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("storage", ["f32", "bf16", "f32_vbf16"])
@pytest.mark.parametrize("D", hd.HEAD_DIMS)
def test_value_mask_twins_are_exact_on_a_poisoned_pyramid(D, storage, route):
    """The masked kernels on a pyramid with NaN in every padding pixel against the oracle on where(mask, value, 0)."""
    name = hd.case_name(D, "p3")
    B, _, _, levels = ec.HEAD_DIM_BASE
    mask = make_mask("bernoulli", B, levels, seed=D)
    assert 0 < int(mask.sum()) < mask.numel()
    vdt, cdt = STORAGE[storage]
    opt, path = ROUTES[route]
    want = hd.expect_info(storage, D)
    with options(value_path=opt):
        for pm, ac in MODES:
            got = run(ec.get_case(name), pm, ac, vdt, cdt, mask=mask)
            info = launch_info()
            assert_exact(got, ec.masked_reference(name, pm, ac, mask.numpy()), f"hd{D}_p3 masked {storage} {route} {pm} {int(ac)}")
            hd.assert_info(info, want, f"hd{D} masked {storage}")
            assert info["value_path"] == path and info["fwd_variant"] == 0, info


# ----------------------------------------------------------------------------------------- forced variants
@pytest.mark.parametrize("storage,D", list(hd.UNIT_FWD), ids=[f"{s}-{d}" for s, d in hd.UNIT_FWD])
def test_one_wave_per_unit_forward_where_it_exists(storage, D):
    """unit_fwd = 2 at D / VEC of 32 and 64 lanes; where D / VEC is no power of two (or the accumulators are float64) the
    option is declined and the 256-thread kernel runs — head_dim_cases.UNIT_FWD says which."""
    variant = hd.UNIT_FWD[(storage, D)]
    want = hd.expect_info(storage, D)
    if variant == 2:
        want.update(fwd_group=D // want["fwd_vec"], fwd_chunks=1)
    with options(unit_fwd=2):
        for kind in ("p3", "c25"):
            info = check(hd.case_name(D, kind), storage, want, f"hd{D}_{kind} {storage} unit_fwd=2")
            assert info["fwd_variant"] == variant, info
    with options(unit_fwd=0):  # ... and the same shapes through the 256-thread kernel: G = 32 / 64 lanes, exactly filled
        info = check(hd.case_name(D, "p3"), storage, hd.expect_info(storage, D), f"hd{D}_p3 {storage} unit_fwd=0")
        assert info["fwd_variant"] == 0, info


@pytest.mark.parametrize("planes", [1, 2], ids=["one_plane", "two_planes"])
@pytest.mark.parametrize("storage,D", list(hd.LDS_LEVELS), ids=[f"{s}-{d}" for s, d in hd.LDS_LEVELS])
def test_lds_served_levels_decline_beyond_sixteen_lanes(storage, D, planes):
    """lds_levels = 2 at G = 32 and G = 64 (Q = 200 as in lds_q200): the LDS-served forward exists up to G = 16 and the
    sample gradients' up to G = 8, so both decline — asserted, not skipped — and the result is exact all the same."""
    fwd, sample = hd.LDS_LEVELS[(storage, D)]
    with options(unit_fwd=0, lds_levels=2, lds_planes=planes):
        info = check(f"hd{D}_lds", storage, hd.expect_info(storage, D), f"hd{D}_lds {storage} planes={planes}")
    assert info["fwd_variant"] == fwd and info["sample_variant"] == sample, info


@pytest.mark.parametrize("storage", ["f32", "f32_vbf16"])
@pytest.mark.parametrize("D", [68, 260])
def test_four_byte_aligned_view_takes_the_scalar_kernels(D, storage):
    """Value rows that start 4 bytes into a 16-byte unit: the forward and the sample gradients run VEC = 1 (68 lanes in two
    chunks, 260 in five) while grad_value, which reads grad_out only, keeps its 16-byte pieces."""
    dense, view = hd.expect_info(storage, D), hd.expect_info(storage, D, aligned=False)
    assert view["fwd_vec"] == 1 and view["sample_vec"] == 1 and view["value_vec"] == 4 and dense["fwd_vec"] == 4
    for kind in ("p3", "c25"):
        check(hd.case_name(D, kind), storage, view, f"hd{D}_{kind} {storage} unaligned", layout="unaligned")
        check(hd.case_name(D, kind), storage, dense, f"hd{D}_{kind} {storage} dense")


# ----------------------------------------------------------------------------------------- the fused module-core families
from msda_triton_amd import _ext, _lib  # noqa: E402
from msda_triton_amd.functional import KernelTimer, fused_hf_box_core, fused_hf_module_core, fused_module_core  # noqa: E402
from test_gpu_fused_ragged import close16  # noqa: E402
from test_gpu_fused_storage import close  # noqa: E402
from test_gpu_parity import BWD_TOL, FWD_TOL  # noqa: E402

DEV = "cuda:0"
FUSED_IDS = [f"{f}-{s}-d{d}-s{n}" for f, s, d, n in hd.fused_case_list()]


def fused_run(inp, pm, ac, cast=None):
    """One forward + backward of the family under KernelTimer; -> (out, grad_value, grad_proj, grad_ref) on the host, the
    launchers' names, the launch info.  cast: run the float32 kernels on the same (rounded) inputs."""
    family = inp["family"]
    v, pr, rf, go = (inp[k] if cast is None else inp[k].to(cast) for k in ("value", "proj", "ref", "gout"))
    if inp["mask"] is not None:  # NaN in every padding pixel
        v = torch.where(inp["mask"][:, :, None, None], v, torch.full_like(v, float("nan")))
    v, pr, rf = (t.to(DEV).requires_grad_(True) for t in (v, pr, rf))
    shapes = inp["shapes"].to(DEV)
    with KernelTimer() as kt:
        if family in ("uniform", "ragged"):
            out = fused_module_core(v, shapes, pr, rf, pm, ac, points_per_level=inp["counts"])
        elif family == "hfbox":
            out = fused_hf_box_core(v, shapes, pr, rf, inp["counts"], 0.5, pm, ac)
        else:
            out = fused_hf_module_core(v, shapes, pr, rf, pm, ac, value_mask=None if inp["mask"] is None else inp["mask"].to(DEV))
        out.backward(go.to(DEV, out.dtype))
        torch.cuda.synchronize()
    return [t.detach().cpu() for t in (out, v.grad, pr.grad, rf.grad)], [r[0] for r in kt.records], launch_info()


def _worst(got, want, atol, rtol):
    """largest |got - want| / (atol + rtol |want|): at most 1 where assert_close passes"""
    got, want = got.double(), want.double()
    return float(((got - want).abs() / (atol + rtol * want.abs())).max())


def assert_16_bit_close(storage, got, w32, sdt, what):
    """A 16-bit storage variant's (out, grad_value, grad_proj, grad_ref) against the float32 kernels' on the same rounded
    inputs, with the bounds of tests/test_gpu_fused_storage.py."""
    out, gv, gp, gr = got
    if storage.startswith("v"):  # 16-bit value rows only: float32 numbers everywhere but grad_value
        torch.testing.assert_close(out, w32[0], atol=2e-5, rtol=1e-4)
        close16(gv, w32[1], sdt, what + " grad_value", scale_tol=3.0)
        torch.testing.assert_close(gp, w32[2], atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(gr, w32[3], atol=1e-3, rtol=1e-3)
    else:
        close(out, w32[0], sdt, what + " out")
        close(gp, w32[2], sdt, what + " grad_proj")
        if storage.startswith("s"):
            close(gv, w32[1], sdt, what + " grad_value", scale_tol=3.0)
            assert gr.dtype == torch.float32
            torch.testing.assert_close(gr, w32[3], rtol=2e-4, atol=2e-4 * float(w32[3].abs().max()))
        else:
            # One 16-bit type for every tensor.  grad_value as the other 16-bit variants': the derived points are
            # parked in float32 for the grad_value passes (ParkType), which are the float pipeline on 16-bit rows.
            close(gv, w32[1], sdt, what + " grad_value", scale_tol=3.0)
            # grad_ref: the per-head partials are rounded to 16 bits and summed, so an element carries half an ulp
            # of EVERY partial, not of itself — norm-wise, with the bound tests/test_gpu_fused_storage.py holds a
            # 16-bit call's reference-point gradients to.
            rel = float((gr.double() - w32[3].double()).norm() / w32[3].double().norm().clamp_min(1e-30))
            assert rel < 2e-2, (what, "grad_ref", rel)


@pytest.mark.parametrize("family,storage,D,S", hd.fused_case_list(), ids=FUSED_IDS)
def test_fused_families_in_the_expected_instantiation(family, storage, D, S):
    """float64 and float32 against the host fp64 module core (1e-8; FWD_TOL / BWD_TOL of tests/test_gpu_parity.py, offsets
    away from grid kinks); 16-bit storage against the float32 kernels on the same rounded inputs with the bounds of
    tests/test_gpu_fused_storage.py.  S = 70 samples per unit are more than a unit has lanes: the lane-strided softmax."""
    want_info = hd.expect_info(hd.FUSED_ARITH[storage], D)
    if storage in hd.SIXTEEN_BIT:  # their grad_value passes are the float32 pipeline on 16-bit rows: VEC = 4
        want_info.update({k: v for k, v in hd.expect_info("f32", D).items() if k.startswith("value_")})
    for ref_dim in hd.fused_ref_dims(family):
        inp = hd.fused_inputs(family, storage, D, S, ref_dim)
        elem = hd.fused_elem_size(storage)
        limit = int(_lib.load().msda_fused_lp_limit(D, elem))
        ext = _ext.load()
        assert S <= limit and (ext is None or int(ext.fused_lp_limit(D, elem)) == limit), (S, limit)  # no composition
        for pm, ac in hd.FUSED_MODES:
            what = f"{family} {storage} D={D} S={S} ref_dim={ref_dim} {pm} {int(ac)}"
            got, names, info = fused_run(inp, pm, ac)
            assert names == hd.FUSED_NAMES[family], (what, names)
            hd.assert_info(info, want_info, what)
            sdt = inp["value"].dtype
            if storage in hd.FUSED_AGAINST_FP64:
                want = hd.fused_reference(inp, pm, ac)
                td = inp["proj"].dtype
                keep = ~torch.from_numpy(hd.fused_kinks(inp, ac))
                assert float((~keep).float().mean()) <= hd.KINK_CAP
                got[2][..., :2] = torch.where(keep, got[2][..., :2], torch.zeros_like(got[2][..., :2]))
                want[2][..., :2] = torch.where(keep, want[2][..., :2], torch.zeros_like(want[2][..., :2]))
                tols = [FWD_TOL[td], BWD_TOL[td], BWD_TOL[td], BWD_TOL[td]]
                print(what, "error / bound:", [round(_worst(g, w, **t), 4) for g, w, t in zip(got, want, tols)])
                for name, g, w, t in zip(("out", "grad_value", "grad_proj", "grad_ref"), got, want, tols):
                    torch.testing.assert_close(g, w.to(td), msg=lambda m: f"{what} {name}: {m}", **t)
                continue
            # 16-bit storage: the float32 kernels on the same rounded inputs
            w32, names32, _ = fused_run(inp, pm, ac, cast=torch.float32)
            assert names32 == hd.FUSED_NAMES[family], (what, names32)
            assert_16_bit_close(storage, got, w32, sdt, what)
