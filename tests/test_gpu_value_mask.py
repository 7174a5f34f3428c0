"""GPU: the value-mask kernels (msda_{fwd,bwd}_masked_<dtype>, msda_{fwd,bwd}_fused_levelref_masked_<suffix>).

The bar is EQUALITY: a masked corner reads 0 exactly where the pre-masked tensor holds 0, the kernels are otherwise their
twins' instruction for instruction, and grad_value does not depend on `value` at all — so the masked kernels on a value
pyramid whose padding pixels hold NaN (or +Inf) must give, bit for bit, what the unmasked kernels of the same library give
on where(mask, value, 0) at the same options.  The CPU oracle on the pre-masked value is held next to it (FWD_TOL / BWD_TOL
of tests/test_gpu_parity.py), so that a fault shared by both GPU routes cannot hide."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

from conftest import MODES, kink_mask
from msda_triton_amd import _ext, _lib, functional
from msda_triton_amd.functional import KernelTimer, fused_hf_module_core, multiscale_deformable_attention
from test_gpu_fused_ragged import SHAPES as FUSED_SHAPES
from test_gpu_lds_levels import CASES as LDS_CASES
from test_gpu_parity import BWD_TOL, DEV, FWD_TOL, SHAPE_MATRIX, rand_case

pytestmark = pytest.mark.gpu

# the smallest shapes at which each code path exists: tests/test_gpu_lds_levels.py's, and one scalar-path shape (D = 5)
CASES = {k: LDS_CASES[k] for k in ("c2_like_f32", "no_level_fits_but_last", "coarse_first_order", "many_samples_two_trips",
                                   "bf16_g4", "fp16_d64", "f64", "d64_f32_g16")}
CASES["d5_scalar"] = SHAPE_MATRIX["d5_scalar"] + (torch.float32,)
MASKS = ("bernoulli", "rect", "element0_masked", "all_ones", "level_edges")


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


def make_mask(kind, B, levels, seed):
    """[B, I] bool on the host, True = real pixel; every mask is seeded"""
    I = sum(h * w for h, w in levels)  # noqa: E741
    g = torch.Generator().manual_seed(seed)
    m = torch.ones(B, I, dtype=torch.bool)
    if kind == "bernoulli":
        m = torch.rand(B, I, generator=g) < 0.5
    elif kind == "rect":  # the padding mask of a batch whose last element is valid on the left 75 % and top 60 % of every level
        start = 0
        for h, w in levels:
            lv = torch.zeros(h, w, dtype=torch.bool)
            lv[:max(1, int(h * 0.6)), :max(1, int(w * 0.75))] = True
            m[B - 1, start:start + h * w] = lv.reshape(-1)
            start += h * w
    elif kind == "element0_masked":
        m[0] = False
    elif kind == "level_edges":  # the last pixel of each level is padding, the first of the next is real: an index off by one shows
        start = 0
        for h, w in levels:
            start += h * w
            m[:, start - 1] = False
    return m


def poisoned(value, m, poison):
    return torch.where(m[:, :, None, None], value, torch.full_like(value, poison))


def premasked(value, m):
    return torch.where(m[:, :, None, None], value, torch.zeros_like(value))


def fwd_bwd(v, s, l, a, go, pm, ac, mask=None):
    v, l, a = (t.detach().clone().requires_grad_(True) for t in (v, l, a))
    out = multiscale_deformable_attention(v, s, l, a, pm, ac, value_mask=mask)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), v.grad, l.grad, a.grad


def tensors(c, td):
    return [torch.from_numpy(c[k]).to(DEV, td) for k in ("value", "loc", "attn", "grad_out")] + [torch.from_numpy(c["shapes"]).to(DEV)]


def assert_contract(got, want, m, what=""):
    """got: the masked kernels on the poisoned value; want: the unmasked kernels on the pre-masked value"""
    assert torch.equal(got[0], want[0]), f"{what} out: max diff {(got[0].double() - want[0].double()).abs().max().item():.3e}"
    gv = torch.where(m[:, :, None, None], want[1], torch.zeros_like(want[1]))
    assert torch.equal(got[1], gv), f"{what} grad_value"
    for nm, x, y in zip(("grad_loc", "grad_attn", "grad_ref"), got[2:], want[2:]):
        assert torch.equal(x, y), f"{what} {nm}: max diff {(x.double() - y.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", list(CASES))
def test_masked_kernels_equal_the_unmasked_kernels_on_the_premasked_value(oracle, name, kind):
    B, Q, H, D, levels, P, td = CASES[name]
    seed = zlib.crc32(f"{name}{kind}".encode())
    c = rand_case(np.random.default_rng(seed), B, Q, H, D, levels, P, dtype=np.float64 if td == torch.float64 else np.float32)
    v, l, a, go, s = tensors(c, td)
    m = make_mask(kind, B, levels, seed).to(DEV)
    vp = poisoned(v, m, float("inf") if kind == "rect" else float("nan"))  # NaN in every masked pixel; +Inf for one mask
    pre = premasked(v, m)
    for pm, ac in MODES:
        ref = {}
        for lds in (0, 2):  # memory-served and LDS-served levels; never the one-wave-per-unit forward
            with options(unit_fwd=0, lds_levels=lds):
                want = fwd_bwd(pre, s, l, a, go, pm, ac)
                info_want = _lib.last_launch_info()
                with KernelTimer() as kt:
                    got_t = fwd_bwd(vp, s, l, a, go, pm, ac, m)
                got = fwd_bwd(vp, s, l, a, go, pm, ac, m)
                info = _lib.last_launch_info()
            what = f"{pm}/{ac} lds_levels={lds}"
            assert_contract(got, want, m, what)
            assert_contract(got_t, want, m, what + " (timed)")
            # the route: the masked call takes the variant its twin takes at these options, never the unit forward
            for k in ("fwd_variant", "fwd_lds_level_bytes", "sample_variant", "value_path", "value_passes"):
                assert info[k] == info_want[k], (what, k, info, info_want)
            assert info["fwd_variant"] == (0 if lds == 0 else info_want["fwd_variant"]) and info["fwd_variant"] in (0, 1)
            if name == "c2_like_f32" and lds == 2:
                assert info["fwd_variant"] == 1 and info["sample_variant"] == 1 and info["fwd_lds_level_bytes"] > 0, info
            names = [r[0] for r in kt.records]
            assert names.count("msda_fwd_masked") == 1 and names.count("msda_bwd_masked_sample") == 1 and \
                names.count("msda_bwd_masked_value") == 1 and len(names) == 3, names
            ref[lds] = got
        for x, y in zip(ref[0], ref[2]):  # (the variants are bit-identical among themselves, as their twins are)
            assert torch.equal(x, y)
        with options(unit_fwd=0):  # the launcher's own choice for a masked call (default options otherwise) is right too
            got = fwd_bwd(vp, s, l, a, go, pm, ac, m)
        assert_contract(got, ref[0], torch.ones_like(m), f"{pm}/{ac} default lds_levels")
        got = fwd_bwd(vp, s, l, a, go, pm, ac, m)  # ... and with every option at its default
        assert _lib.last_launch_info()["fwd_variant"] in (0, 1)
        for x, y in zip(got[1:], ref[0][1:]):
            assert torch.equal(x, y)
        assert torch.equal(got[0], ref[0][0])
        if kind == "all_ones":  # equals the unmasked call on the raw value
            with options(unit_fwd=0):
                raw = fwd_bwd(v, s, l, a, go, pm, ac)
            for x, y in zip(ref[0], raw):
                assert torch.equal(x, y)
        if kind in ("bernoulli", "rect"):  # the mask has an effect: not what the padding pixels replaced by ones give
            ones = fwd_bwd(poisoned(v, m, 1.0), s, l, a, go, pm, ac)
            assert not torch.equal(ones[0], ref[0][0])
        if td in FWD_TOL:  # the CPU oracle on the pre-masked value
            host = premasked(torch.from_numpy(c["value"]), m.cpu()).numpy()
            r_out = oracle.forward(host, c["shapes"], c["loc"], c["attn"], pm, ac)
            r_gv, r_gl, r_ga = oracle.backward(c["grad_out"], host, c["shapes"], c["loc"], c["attn"], pm, ac)
            out, gv, gl, ga = (t.cpu().numpy() for t in ref[2])
            np.testing.assert_allclose(out, r_out, err_msg="out", **FWD_TOL[td])
            np.testing.assert_allclose(gv, np.where(m.cpu().numpy()[:, :, None, None], r_gv, 0), err_msg="grad_value", **BWD_TOL[td])
            np.testing.assert_allclose(ga, r_ga, err_msg="grad_attn", **BWD_TOL[td])
            keep = ~kink_mask(c["loc"], c["shapes"], ac)
            np.testing.assert_allclose(np.where(keep, gl, 0), np.where(keep, r_gl, 0), err_msg="grad_loc", **BWD_TOL[td])


# (two passes over the batch: the shapes with B >= 2)
ROUTES = [(n, 2, 1) for n in ("c2_like_f32", "bf16_g4", "fp16_d64", "f64", "d5_scalar")] + \
         [(n, 2, 2) for n in ("c2_like_f32", "bf16_g4", "d5_scalar")] + \
         [(n, 3, 1) for n in ("c2_like_f32", "bf16_g4", "fp16_d64", "f64", "d5_scalar")]


@pytest.mark.parametrize("rig", [0, 1], ids=["records_in_workspace", "records_in_grads"])
@pytest.mark.parametrize("name,path,passes", ROUTES,
                         ids=[f"{n}-{'single_launch' if p == 3 else 'sorted'}{'_two_passes' if k == 2 else ''}" for n, p, k in ROUTES])
def test_both_grad_value_routes_store_the_padding_rows_as_zeros(name, path, passes, rig):
    B, Q, H, D, levels, P, td = CASES[name]
    assert passes <= B
    seed = zlib.crc32(name.encode()) + 7
    c = rand_case(np.random.default_rng(seed), B, Q, H, D, levels, P, dtype=np.float64 if td == torch.float64 else np.float32)
    v, l, a, go, s = tensors(c, td)
    for kind in ("bernoulli", "level_edges", "element0_masked"):
        m = make_mask(kind, B, levels, seed).to(DEV)
        with options(unit_fwd=0, value_path=path, ws_passes=passes, records_in_grads=rig):
            want = fwd_bwd(premasked(v, m), s, l, a, go, "zeros", False)
            info_want = _lib.last_launch_info()
            got = fwd_bwd(poisoned(v, m, float("nan")), s, l, a, go, "zeros", False, m)
            info = _lib.last_launch_info()
        assert info["value_path"] == (1 if path == 3 else 2) and info["value_passes"] == passes, info
        assert info_want["value_path"] == info["value_path"] and info_want["value_passes"] == passes
        assert_contract(got, want, m, kind)
        assert not torch.signbit(got[1][~m]).any()  # +0


# ------------------------------------------------------------------------------------------ the fused pair
# (under KernelTimer the masked fused pair keeps its twin's launcher-level names: that the MASKED symbols ran shows in the
#  results — the unmasked kernels would carry the planted NaN into every output — together with `no_composition`, under
#  which a masked_fill of the package's own raises)
@contextlib.contextmanager
def no_composition(calls=None):
    real = functional.apply_value_mask

    def spy(img, value_mask):
        if value_mask is not None:
            if calls is None:
                raise AssertionError("the mask was composed as masked_fill instead of going into the kernels")
            calls.append(1)
        return real(img, value_mask)

    functional.apply_value_mask = spy
    try:
        yield
    finally:
        functional.apply_value_mask = real


FUSED_NAMES = ["msda_fwd_fused_levelref", "msda_bwd_fused_levelref"]


def fused_run(v, s, pr, rf, go, pm, ac, mask=None, **kw):
    v, pr, rf = (t.detach().clone().requires_grad_(True) for t in (v, pr, rf))
    out = fused_hf_module_core(v, s, pr, rf, pm, ac, value_mask=mask, **kw)
    out.backward(go.to(out.dtype))
    torch.cuda.synchronize()
    return out.detach(), v.grad, pr.grad, rf.grad


def fused_inputs(B, Q, H, D, levels, P, ref_dim, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=dtype)
    proj = torch.randn(B, Q, H, len(levels), P, 3, generator=g, dtype=dtype) * 1.5
    ref = torch.rand(B, Q, len(levels), ref_dim, generator=g, dtype=dtype)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=dtype)
    return [t.to(DEV) for t in (value, torch.tensor(levels), proj, ref, gout)]


@pytest.mark.parametrize("pm,ac", [("zeros", False), ("border", True)], ids=["zeros_0", "border_1"])
@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("name", ["d32", "d5", "d64"])
def test_fused_pair_equals_the_unmasked_fused_kernels_on_the_premasked_value(name, ref_dim, P, pm, ac):
    B, Q, H, D, levels = FUSED_SHAPES[name]
    seed = zlib.crc32(f"{name}{ref_dim}{P}".encode())
    v, s, pr, rf, go = fused_inputs(B, Q, H, D, levels, P, ref_dim, seed)
    for kind in ("bernoulli", "rect", "level_edges"):
        m = make_mask(kind, B, levels, seed).to(DEV)
        vp = poisoned(v, m, float("nan"))
        for lds in (0, 2):
            with options(lds_levels=lds):
                with KernelTimer() as kt:
                    want = fused_run(premasked(v, m), s, pr, rf, go, pm, ac)
                assert [r[0] for r in kt.records] == FUSED_NAMES
                with KernelTimer() as kt, no_composition():
                    got = fused_run(vp, s, pr, rf, go, pm, ac, m)
                assert [r[0] for r in kt.records] == FUSED_NAMES and torch.isfinite(got[0]).all()
                assert_contract(got, want, m, f"{kind} lds_levels={lds}")
                # the Python Function outside the timer and the composition agree bit for bit as well
                assert_contract(fused_run(vp, s, pr, rf, go, pm, ac, m), want, m, kind)
                comp = fused_run(vp, s, pr, rf, go, pm, ac, m, mask_in_kernels=False)
                if _ext.load() is None:  # (with the C++ node the unmasked call reduces grad_ref in another order: closeness)
                    assert_contract(comp, want, m, kind + " composed")
                else:
                    assert torch.equal(comp[0], want[0]) and torch.equal(comp[1], got[1]) and torch.equal(comp[2], want[2])
                    torch.testing.assert_close(comp[3], want[3], atol=1e-4, rtol=1e-4)


def test_fused_pair_through_ctypes_agrees_with_the_function():
    """the ctypes launch of the masked fused pair (msda_hip_fwd_fused / msda_hip_bwd_fused) against the autograd Function"""
    B, Q, H, D, levels = FUSED_SHAPES["d32"]
    v, s, pr, rf, go = fused_inputs(B, Q, H, D, levels, 4, 2, 5)
    m = make_mask("bernoulli", B, levels, 5).to(DEV)
    vp = poisoned(v, m, float("nan"))
    got = fused_run(vp, s, pr, rf, go, "zeros", False, m)
    out = functional.msda_hip_fwd_fused(vp, s, pr, rf, "zeros", False, levelref=True, value_mask=m)
    g_img, g_proj, g_ref = functional.msda_hip_bwd_fused(go, vp, s, pr, rf, "zeros", False, levelref=True, value_mask=m)
    for x, y in zip(got, (out, g_img, g_proj, g_ref)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("sdt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_storage_variants(sdt, ref_dim):
    """_vbf16 / _vf16 (16-bit value), _sbf16 / _sf16 (16-bit value and projection) and the all-16-bit instantiation, at the
    shape of test_gpu_hf_fused.test_storage_variants_match_fp32_on_the_rounded_inputs"""
    levels = [(20, 16), (10, 8), (5, 4)]
    B, Q, H, D, P = 2, 90, 4, 32, 4
    v, s, pr, rf, go = fused_inputs(B, Q, H, D, levels, P, ref_dim, 31 + ref_dim)
    m = make_mask("rect", B, levels, 3).to(DEV)
    v16, pr16, go16 = v.to(sdt), pr.to(sdt), go.to(sdt)
    for vv, pp, rr, gg in ((v16, pr, rf, go), (v16, pr16, rf, go16), (v16, pr16, rf.to(sdt), go16)):
        want = fused_run(premasked(vv, m), s, pp, rr, gg, "zeros", False)
        with KernelTimer() as kt, no_composition():
            got = fused_run(poisoned(vv, m, float("nan")), s, pp, rr, gg, "zeros", False, m)
        assert [r[0] for r in kt.records] == FUSED_NAMES and torch.isfinite(got[0].float()).all()
        assert_contract(got, want, m, f"{vv.dtype}/{pp.dtype}/{rr.dtype}")


def test_mixed_storage_plain_operator():
    """16-bit value next to fp32 sampling inputs (msda_*_masked_f32_vbf16 / _vf16)"""
    B, Q, H, D, levels, P, _ = CASES["c2_like_f32"]
    c = rand_case(np.random.default_rng(11), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, torch.float32)
    m = make_mask("bernoulli", B, levels, 11).to(DEV)
    for sdt in (torch.bfloat16, torch.float16):
        v16 = v.to(sdt)
        with options(unit_fwd=0):
            want = fwd_bwd(premasked(v16, m), s, l, a, go, "zeros", False)
            got = fwd_bwd(poisoned(v16, m, float("nan")), s, l, a, go, "zeros", False, m)
        assert got[1].dtype == sdt
        assert_contract(got, want, m, str(sdt))


# ------------------------------------------------------------------------------------------ other checks
def test_padded_value_rows_the_mask_indexes_pixels():
    B, Q, H, D, levels, P, td = CASES["c2_like_f32"]
    c = rand_case(np.random.default_rng(5), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    m = make_mask("bernoulli", B, levels, 5).to(DEV)
    vp = poisoned(v, m, float("nan"))
    padded = functional.padded_value_rows(*v.shape, v.dtype, v.device, pad_bytes=128)
    padded.copy_(vp)
    assert not padded.is_contiguous()
    with options(unit_fwd=0):
        want = fwd_bwd(premasked(v, m), s, l, a, go, "zeros", False)
        leaf = padded.detach().requires_grad_(True)
        l2, a2 = l.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = multiscale_deformable_attention(leaf, s, l2, a2, "zeros", False, value_mask=m)
        out.backward(go)
    assert_contract((out.detach(), leaf.grad, l2.grad, a2.grad), want, m)


def test_torch_compile_fullgraph_with_a_mask():
    B, Q, H, D, levels, P, td = CASES["coarse_first_order"]
    c = rand_case(np.random.default_rng(3), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    m = make_mask("bernoulli", B, levels, 3).to(DEV)

    def f(v_, l_, a_, m_):
        return multiscale_deformable_attention(v_, s, l_, a_, "zeros", False, value_mask=m_)

    want = multiscale_deformable_attention(premasked(v, m), s, l, a, "zeros", False)
    got = torch.compile(f, fullgraph=True)(poisoned(v, m, float("nan")), l, a, m)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)


def test_bad_masks_on_the_gpu_raise_value_error():
    B, Q, H, D, levels, P, td = CASES["coarse_first_order"]
    c = rand_case(np.random.default_rng(3), B, Q, H, D, levels, P)
    v, l, a, go, s = tensors(c, td)
    I = v.shape[1]  # noqa: E741
    for bad in (torch.ones(B, I, device=DEV), torch.ones(B, I, 1, dtype=torch.bool, device=DEV), torch.ones(B, I, dtype=torch.bool)):
        with pytest.raises(ValueError):
            multiscale_deformable_attention(v, s, l, a, "zeros", False, value_mask=bad)


def test_wrapped_deformable_detr_training_step_with_a_padding_mask():
    """One training step of the tiny Deformable-DETR of tests/test_hf_model.py on the GPU, fused wrapper, a pixel_mask that
    pads one image: against transformers' own core at that file's bounds — with the mask in the kernels and with the
    adapter's own routing."""
    pytest.importorskip("transformers")
    from test_hf_model import WATCHED, _inputs, run_model, tiny_deformable_detr
    from msda_triton_amd import hf_adapter
    model = tiny_deformable_detr().to(DEV)
    x, mask = _inputs(DEV)
    assert not mask[1].all()
    hs0, enc0, g0 = run_model(model, x, mask)
    assert hf_adapter.replace_hf_msda(model, fused=True) == 8
    keep = hf_adapter.MASK_IN_KERNELS
    try:
        for in_kernels in (True, keep):
            hf_adapter.MASK_IN_KERNELS = in_kernels
            composed = []
            with KernelTimer() as kt, no_composition(composed):
                hs1, enc1, g1 = run_model(model, x, mask)
                torch.cuda.synchronize()
            names = [r[0] for r in kt.records]
            assert names.count("msda_fwd_fused_levelref") == 4 and names.count("msda_bwd_fused_levelref") == 4, names
            assert len(composed) == (0 if in_kernels else 4), (in_kernels, composed)  # masked_fill only where the switch says so
            torch.testing.assert_close(enc1, enc0, atol=1e-4, rtol=1e-3)
            torch.testing.assert_close(hs1, hs0, atol=1e-4, rtol=1e-3)
            for k in WATCHED:
                err = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30))
                assert err < 2e-3, (k, err)
    finally:
        hf_adapter.MASK_IN_KERNELS = keep
