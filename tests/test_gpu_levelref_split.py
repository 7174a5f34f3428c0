"""GPU tests of the per-level-reference fused pair on SPLIT projections (msda_*_fused_levelref_split_<suffix>,
``functional.fused_hf_module_core_split``, the Hugging Face adapter's route for projection layers that are not plain).

The kernels differ from the interleaved pair's in three loads and three stores, so the main check is an EQUALITY with that
pair on the stacked projection (``torch.equal``: no tolerance).  The other bounds are borrowed, not chosen here:
tests/test_gpu_parity.py's FWD_TOL / BWD_TOL against the CPU oracle, tests/test_gpu_fused_ragged.py's ``assert_fp32_close``
for the adapter against transformers' own forward on the same GPU, tests/test_hf_model.py's relative L2 bound under bf16
autocast (both sides carry bf16 round-off)."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

from conftest import kink_mask
from guarded_alloc import contract_violations
from msda_triton_amd import _lib, functional, hf_adapter
from msda_triton_amd.functional import (KernelTimer, fused_hf_module_core, fused_hf_module_core_split,
                                        hf_module_sampling_inputs, msda_hip_bwd_fused, msda_hip_bwd_fused_split,
                                        msda_hip_fwd_fused, msda_hip_fwd_fused_split, padded_value_rows,
                                        stack_split_projection)
from test_gpu_fused_ragged import SHAPES, assert_fp32_close, names
from test_gpu_lds_levels import CASES
from test_gpu_parity import BWD_TOL, FWD_TOL
from test_levelref_split import (assert_same_call, detr_attention, detr_call, make_not_plain, pixel_decoder_call,
                                 pixel_decoder_layer, run_attention)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
# suffix: (value, projection / out, reference points) dtypes
STORAGE = {"f32": (F32, F32, F32), "f16": (F16, F16, F16), "bf16": (BF16, BF16, BF16), "f64": (F64, F64, F64),
           "f32_vbf16": (BF16, F32, F32), "f32_vf16": (F16, F32, F32), "f32_sbf16": (BF16, BF16, F32),
           "f32_sf16": (F16, F16, F32)}
SUFFIX_OF = {F32: "f32", BF16: "bf16", F16: "f16", F64: "f64"}
MODES2 = [("zeros", False, 2), ("border", True, 4)]  # both padding / align pairs, one ref_dim each ...
MODES2X = MODES2 + [("zeros", False, 4), ("border", True, 2)]  # ... and the other way round where the case is cheap
# scalar path (D = 5), several channel chunks (D = 65), the 16-byte path in one chunk
EXTRA = {"d5": SHAPES["d5"], "d65": (2, 21, 2, 65, [(7, 5), (4, 3), (2, 2)]), "d32": SHAPES["d32"]}


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


@contextlib.contextmanager
def spied_symbols(log):
    """records every call of a split entry point of the loaded library"""
    lib = _lib.load()
    real = {n: getattr(lib, n) for n in _lib.LEVELREF_SPLIT_SYMBOLS}

    def spy(n):
        def call(*a):
            log.append(n)
            return real[n](*a)
        return call

    for n in real:
        setattr(lib, n, spy(n))
    try:
        yield
    finally:
        for n in real:
            setattr(lib, n, real[n])


def make(B, Q, H, D, levels, P, ref_dim, seed, suffix="f32", pad_rows=False):
    vdt, pdt, rdt = STORAGE[suffix]
    g = torch.Generator(device="cpu").manual_seed(seed)
    L, I = len(levels), sum(h * w for h, w in levels)  # noqa: E741
    value = torch.randn(B, I, H, D, generator=g, dtype=torch.float64).to(vdt).to(DEV)
    off = (torch.randn(B, Q, H, L, P, 2, generator=g, dtype=torch.float64) * 1.5).to(pdt).to(DEV)
    lgt = (torch.randn(B, Q, H, L, P, generator=g, dtype=torch.float64) * 1.5).to(pdt).to(DEV)
    ref = torch.rand(B, Q, L, ref_dim, generator=g, dtype=torch.float64).to(rdt).to(DEV)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=torch.float64).to(pdt).to(DEV)
    if pad_rows:  # pixel rows a 128-byte line apart (value_row_stride)
        vp = padded_value_rows(B, I, H, D, vdt, DEV, pad_bytes=128)
        vp.copy_(value)
        value = vp
    return value, torch.tensor(levels, device=DEV), off, lgt, ref, gout


def split_launch(value, shapes, off, lgt, ref, gout, pm, ac, level_cells=0):
    out = msda_hip_fwd_fused_split(value, shapes, off, lgt, ref, pm, ac)
    if out is None:
        return None
    res = msda_hip_bwd_fused_split(gout, value, shapes, off, lgt, ref, pm, ac, level_cells=level_cells)
    if res is None:  # (the backward parks more per sample: its own limit on L * P is below the forward's)
        return (out,)
    return (out,) + tuple(res)


def twin_launch(value, shapes, off, lgt, ref, gout, pm, ac, level_cells=0):
    proj = stack_split_projection(off, lgt)
    out = msda_hip_fwd_fused(value, shapes, proj, ref, pm, ac, levelref=True)
    if out is None:
        return None
    res = msda_hip_bwd_fused(gout, value, shapes, proj, ref, pm, ac, level_cells=level_cells, levelref=True)
    if res is None:
        return (out,)
    gv, gp, gr = res
    return out, gv, gp[..., :2].contiguous(), gp[..., 2].contiguous(), gr


WHAT = ("out", "grad_value", "grad_offsets", "grad_logits", "grad_ref")


def assert_bitwise(got, want, where=""):
    assert (got is None) == (want is None), where
    if got is None:
        return False
    assert len(got) == len(want), (where, len(got), len(want))  # (a backward one pair declines, the other declines too)
    for nm, a, b in zip(WHAT, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, (where, nm, a.shape, b.shape, a.dtype, b.dtype)
        assert torch.equal(a, b), (where, nm, float((a.double() - b.double()).abs().max()))
        assert bool(torch.isfinite(a).all()), (where, nm)
    return True


# ------------------------------------------------------------------------------------------------ equality with the twin
@pytest.mark.parametrize("planes", [(0, 1), (2, 1), (2, 2)], ids=["plain", "lds_levels", "two_planes"])
@pytest.mark.parametrize("pm,ac,ref_dim", MODES2, ids=["zeros_0_ref2", "border_1_ref4"])
@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_equal_to_the_interleaved_pair_on_the_lds_level_cases(name, pm, ac, ref_dim, planes):
    B, Q, H, D, levels, P, td = CASES[name]
    c = make(B, Q, H, D, levels, P, ref_dim, zlib.crc32(name.encode()) + ref_dim, SUFFIX_OF[td])
    with options(lds_levels=planes[0], lds_planes=planes[1], unit_fwd=0):
        got = split_launch(*c, pm, ac)
        info = _lib.last_launch_info()
        want = twin_launch(*c, pm, ac)
        twin_info = _lib.last_launch_info()
    ran = assert_bitwise(got, want, (name, planes))
    assert ran and (len(got) == 5 or name == "many_samples_two_trips"), (name, len(got))
    if ran:  # msda_last_launch_info reports the twin's variants
        for k in ("fwd_variant", "fwd_lds_level_bytes", "fwd_lds_planes", "sample_variant", "sample_lds_level_bytes",
                  "value_path", "fwd_vec", "fwd_group", "sample_vec", "sample_group"):
            assert info[k] == twin_info[k], (k, info, twin_info)
    if name == "c2_like_f32" and planes[0] == 2:
        assert ran and info["fwd_variant"] == 1 and info["sample_variant"] == 1 and info["fwd_lds_planes"] == planes[1], info


@pytest.mark.parametrize("route", ["sorted", "sorted_two_passes", "single_launch"])
@pytest.mark.parametrize("shape", list(EXTRA))
@pytest.mark.parametrize("suffix", list(STORAGE))
def test_bitwise_equal_for_every_suffix_on_both_grad_value_routes(suffix, shape, route):
    B, Q, H, D, levels = EXTRA[shape]
    opts = {"sorted": dict(value_path=2), "sorted_two_passes": dict(value_path=2, ws_passes=2),
            "single_launch": dict(value_path=3)}[route]
    for pm, ac, ref_dim in MODES2X:
        c = make(B, Q, H, D, levels, 3, ref_dim, zlib.crc32(f"{suffix}{shape}".encode()) + ref_dim, suffix)
        with options(**opts):
            got = split_launch(*c, pm, ac)
            info = _lib.last_launch_info()
            want = twin_launch(*c, pm, ac)
        assert assert_bitwise(got, want, (suffix, shape, route, pm, ac, ref_dim))
        assert info["value_path"] == (1 if route == "single_launch" else 2), info
        assert info["value_passes"] == (2 if route == "sorted_two_passes" else 1), info
        if shape == "d5":
            assert info["fwd_vec"] == 1 and info["sample_vec"] == 1, info
        if shape == "d65":
            assert info["fwd_chunks"] > 1 and info["sample_chunks"] > 1, info


@pytest.mark.parametrize("suffix", ["f32", "f32_sbf16", "f32_vf16", "f64"])
@pytest.mark.parametrize("lds", [0, 2])
def test_bitwise_equal_on_padded_value_rows(suffix, lds):
    B, Q, H, D, levels, P, _ = CASES["all_levels_fit"]
    for pm, ac, ref_dim in MODES2:
        c = make(B, Q, H, D, levels, P, ref_dim, 41 + ref_dim, suffix, pad_rows=True)
        assert c[0].stride(1) * c[0].element_size() == H * D * c[0].element_size() + 128
        with options(lds_levels=lds, unit_fwd=0):
            got, want = split_launch(*c, pm, ac), twin_launch(*c, pm, ac)
        assert assert_bitwise(got, want, (suffix, lds, pm))
        dense = (c[0].contiguous(),) + c[1:]
        with options(lds_levels=lds, unit_fwd=0):
            assert assert_bitwise(split_launch(*dense, pm, ac), got, (suffix, lds, pm, "dense"))


def test_at_the_fused_limit_and_above_it():
    D, H = 8, 2
    limit = int(_lib.load().msda_fused_lp_limit(D, 4))
    levels = [(6, 5), (3, 4)]
    assert limit % 2 == 0 or limit > 2
    P = limit // 2
    c = make(1, 5, H, D, levels, P, 4, 77)
    log = []
    with spied_symbols(log):
        got = split_launch(*c, "border", False)
    assert 2 * P <= limit and assert_bitwise(got, twin_launch(*c, "border", False), "at the limit")
    assert log == ["msda_fwd_fused_levelref_split_f32", "msda_bwd_fused_levelref_split_f32"]
    # one above: msda_fused_lp_limit is the BACKWARD's bound (it parks more per sample than the forward) — the backward
    # entry point declines before anything is launched, as its twin does; the core composes and neither symbol runs
    P = limit // 2 + 1
    c = make(1, 5, H, D, levels, P, 4, 78)
    assert 2 * P > limit
    assert msda_hip_bwd_fused_split(c[5], *c[:5], "border", False, need_img=False) is None
    assert msda_hip_bwd_fused(c[5], c[0], c[1], stack_split_projection(c[2], c[3]), c[4], "border", False, need_img=False,
                              levelref=True) is None
    log = []
    leaves = [t.clone().requires_grad_(True) for t in (c[0], c[2], c[3], c[4])]
    with spied_symbols(log), KernelTimer() as kt:
        out = fused_hf_module_core_split(leaves[0], c[1], leaves[1], leaves[2], leaves[3], "border", False)
        out.backward(c[5])
    assert not log and not [n for n in names(kt) if "split" in n], (log, names(kt))
    twin = [t.clone().requires_grad_(True) for t in (c[0], c[2], c[3], c[4])]
    want = fused_hf_module_core(twin[0], c[1], stack_split_projection(twin[1], twin[2]), twin[3], "border", False)
    want.backward(c[5])
    assert torch.equal(out, want)
    for a, b in zip(leaves, twin):
        assert torch.equal(a.grad, b.grad)


# ------------------------------------------------------------------------------------------------ the core
def run_core(split, value, shapes, off, lgt, ref, gout, pm, ac, **kw):
    leaves = [t.detach().clone().requires_grad_(True) for t in (value, off, lgt, ref)]
    if split:
        out = fused_hf_module_core_split(leaves[0], shapes, leaves[1], leaves[2], leaves[3], pm, ac, **kw)
    else:
        out = fused_hf_module_core(leaves[0], shapes, stack_split_projection(leaves[1], leaves[2]), leaves[3], pm, ac, **kw)
    out.backward(gout.to(out.dtype))
    return (out.detach(),) + tuple(t.grad for t in leaves)


@pytest.mark.parametrize("pm,ac,ref_dim", MODES2X, ids=["zeros_0_ref2", "border_1_ref4", "zeros_0_ref4", "border_1_ref2"])
def test_route_one_forward_and_one_backward_symbol_nothing_composed(monkeypatch, pm, ac, ref_dim):
    B, Q, H, D, levels = SHAPES["d32"]
    c = make(B, Q, H, D, levels, 4, ref_dim, 5 + ref_dim)
    log = []
    monkeypatch.setattr(functional, "stack_split_projection", lambda *a: pytest.fail("the projections were interleaved"))
    with spied_symbols(log), KernelTimer() as kt:
        got = run_core(True, *c, pm, ac)
    assert log == ["msda_fwd_fused_levelref_split_f32", "msda_bwd_fused_levelref_split_f32"], log
    assert names(kt) == ["msda_fwd_fused_levelref_split", "msda_bwd_fused_levelref_split"], names(kt)
    monkeypatch.undo()
    assert assert_bitwise(got, run_core(False, *c, pm, ac), "core")
    # the layers' flat layouts are views: the same kernels, the same bits
    flat = (c[0], c[1], c[2].reshape(B, Q, -1), c[3].reshape(B, Q, H, -1)) + c[4:]
    again = run_core(True, *flat, pm, ac)
    assert torch.equal(again[0], got[0]) and torch.equal(again[2].reshape(got[2].shape), got[2])
    assert torch.equal(again[3].reshape(got[3].shape), got[3])
    # masks compose around the kernels
    g = torch.Generator().manual_seed(3)
    vm, qm = (torch.rand(B, c[0].shape[1], generator=g) > 0.2).to(DEV), (torch.rand(B, Q, generator=g) > 0.3).to(DEV)
    log = []
    with spied_symbols(log):
        masked = run_core(True, *c, pm, ac, value_mask=vm, query_mask=qm)
    assert len(log) == 2
    assert_fp32_close(masked, run_core(False, *c, pm, ac, value_mask=vm, query_mask=qm, mask_in_kernels=False))
    assert not masked[0][~qm].any() and not masked[1][~vm].any() and not masked[2][~qm].any() and not masked[3][~qm].any()


def test_option_profile_names_the_launches():
    c = make(*SHAPES["d8"][:5], 4, 2, 9)
    with options(profile=1):
        _lib.profile_read()
        split_launch(*c, "zeros", False)
        torch.cuda.synchronize()
        prof = _lib.profile_read()
    assert prof["msda_fwd_fused_levelref_split"][0] == 1 and prof["msda_bwd_fused_levelref_split"][0] == 1, prof
    assert "msda_fwd_kernel" not in prof and "msda_bwd_sample_kernel" not in prof, prof


@pytest.mark.parametrize("pm,ac,ref_dim", MODES2X, ids=["zeros_0_ref2", "border_1_ref4", "zeros_0_ref4", "border_1_ref2"])
@pytest.mark.parametrize("td", [F32, F64], ids=["fp32", "fp64"])
def test_against_the_cpu_oracle_behind_the_prologue(oracle, td, pm, ac, ref_dim):
    """out, grad_value and, chained through transformers' prologue by host autograd, the gradients of both projections and
    of the reference points — at tests/test_gpu_parity.py's bounds; location gradients within 1e-4 px of a pixel boundary
    (where either side is legitimate) are left out, as there."""
    B, Q, H, D, levels = 2, 41, 3, 8, [(9, 7), (5, 6), (3, 2)]
    c = make(B, Q, H, D, levels, 3, ref_dim, 11 + ref_dim, SUFFIX_OF[td])
    got = [t.cpu() for t in run_core(True, *c, pm, ac)]
    value, shapes, off, lgt, ref, gout = (t.cpu() for t in c)
    leaves = [t.clone().requires_grad_(True) for t in (off, lgt, ref)]
    pts, att = hf_module_sampling_inputs(stack_split_projection(leaves[0], leaves[1]), shapes, leaves[2])
    v, s, p, a, go = value.numpy(), shapes.numpy(), pts.detach().numpy(), att.detach().numpy(), gout.numpy()
    r_out = oracle.forward(v, s, p, a, pm, ac)
    r_gv, r_gl, r_ga = oracle.backward(go, v, s, p, a, pm, ac)
    kink = kink_mask(p, s, ac)
    gl = torch.from_numpy(np.where(kink, 0, np.asarray(r_gl))).to(td)
    r_off, r_lgt, r_ref = torch.autograd.grad([pts, att], leaves, [gl, torch.from_numpy(np.asarray(r_ga)).to(td)])
    np.testing.assert_allclose(got[0].numpy(), r_out, **FWD_TOL[td])
    np.testing.assert_allclose(got[1].numpy(), r_gv, **BWD_TOL[td])
    np.testing.assert_allclose(got[3].numpy(), r_lgt.numpy(), **BWD_TOL[td])
    np.testing.assert_allclose(np.where(kink, 0, got[2].numpy()), r_off.numpy(), **BWD_TOL[td])
    # a level's reference point sums its samples' location gradients over heads and points: entries with a kink among them out
    dirty = torch.from_numpy(kink).any(-1).any(-1).any(2)[..., None].expand(B, Q, len(levels), ref_dim).numpy()  # [B, Q, L]
    assert dirty.mean() < 0.5
    np.testing.assert_allclose(np.where(dirty, 0, got[4].numpy()), np.where(dirty, 0, r_ref.numpy()), **BWD_TOL[td])


@pytest.mark.parametrize("route", ["sorted", "single_launch"])
@pytest.mark.parametrize("suffix", ["f32", "f32_sbf16", "f64"])
def test_buffer_contract_and_every_gradient_element_written(suffix, route):
    """guarded_alloc's three runs of the two launchers: bands intact, out / grad_value / both projection gradients / the
    partials' sum bit-identical whatever the pre-fill (0xFF is a NaN in every float type here), no byte left unwritten."""
    B, Q, H, D, levels = SHAPES["d8"]
    c = make(B, Q, H, D, levels, 3, 4, 19, suffix)
    with options(value_path=2 if route == "sorted" else 3):
        bad, rigs, _ = contract_violations(lambda: msda_hip_fwd_fused_split(*c[:5], "zeros", False), 1, DEV, names=["out"])
        assert not bad, bad
        # grad_value, grad_offsets, grad_logits, the partials, (sorted: the workspace)
        call = lambda: msda_hip_bwd_fused_split(c[5], *c[:5], "zeros", False)  # noqa: E731
        bad, rigs, res = contract_violations(call, 5, DEV, names=list(WHAT[1:]))
        assert not bad, bad
        shapes = [a["shape"] for a in rigs[0].allocations]
        assert (B, Q, H, len(levels), 3, 2) in shapes and (B, Q, H, len(levels), 3) in shapes, shapes


def test_two_runs_are_identical():
    B, Q, H, D, levels, P, _ = CASES["odd_points_boundary"]
    c = make(B, Q, H, D, levels, P, 4, 23)
    for opts in (dict(value_path=2), dict(value_path=3), dict(value_path=2, lds_levels=2, unit_fwd=0)):
        with options(**opts):
            assert assert_bitwise(split_launch(*c, "zeros", False), split_launch(*c, "zeros", False), opts)


# ------------------------------------------------------------------------------------------------ the HF adapter
@pytest.mark.parametrize("how", ["lora", "hook"])
def test_adapter_takes_the_split_symbols_behind_layers_that_are_not_plain(how):
    for ref_dim in (2, 4):
        holder = torch.nn.ModuleDict({"attn": detr_attention()})
        make_not_plain(holder["attn"], how)
        holder.to(DEV)
        hidden, kw = detr_call(DEV, ref_dim=ref_dim)
        want = run_attention(holder["attn"], hidden, kw)  # transformers' own forward on the GPU
        assert hf_adapter.replace_hf_msda(holder, fused=True) == 2
        log = []
        with spied_symbols(log):
            got = run_attention(holder["attn"], hidden, kw)
        assert log == ["msda_fwd_fused_levelref_split_f32", "msda_bwd_fused_levelref_split_f32"], log
        assert_fp32_close((got[0],) + tuple(got[1][k] for k in sorted(got[1])),
                          (want[0],) + tuple(want[1][k] for k in sorted(want[1])))
        assert_same_call(got, want, atol=2e-5, rtol=1e-4, gtol=1e-4)


def test_adapter_plain_layers_still_launch_the_interleaved_kernels():
    holder = torch.nn.ModuleDict({"attn": detr_attention()}).to(DEV)
    hidden, kw = detr_call(DEV)
    want = run_attention(holder["attn"], hidden, kw)
    hf_adapter.replace_hf_msda(holder, fused=True)
    log = []
    with spied_symbols(log), KernelTimer() as kt:
        got = run_attention(holder["attn"], hidden, kw)
    assert not log and names(kt).count("msda_fwd_fused_levelref") == 1 and names(kt).count("msda_bwd_fused_levelref") == 1
    assert_same_call(got, want, atol=2e-5, rtol=1e-4, gtol=1e-4)


def test_adapter_bf16_autocast_through_the_split_route():
    """both sides carry bf16 round-off: the relative L2 bound tests/test_hf_model.py uses under bf16 autocast, measured
    against how far bf16 autocast itself is from fp32"""
    holder = torch.nn.ModuleDict({"attn": detr_attention()})
    make_not_plain(holder["attn"], "lora")
    holder.to(DEV)
    hidden, kw = detr_call(DEV)
    fp32 = run_attention(holder["attn"], hidden, kw)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        want = run_attention(holder["attn"], hidden, kw)
    hf_adapter.replace_hf_msda(holder, fused=True)
    log = []
    with spied_symbols(log), torch.autocast("cuda", dtype=torch.bfloat16):
        got = run_attention(holder["attn"], hidden, kw)
    assert log == ["msda_fwd_fused_levelref_split_f32_sbf16", "msda_bwd_fused_levelref_split_f32_sbf16"], log
    rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-12))  # noqa: E731
    noise = rel(want[0], fp32[0])
    assert rel(got[0], want[0]) < max(3 * noise, 3e-2), (rel(got[0], want[0]), noise)
    for k in want[1]:
        assert torch.isfinite(got[1][k]).all()
        assert rel(got[1][k], want[1][k]) < 0.15, (k, rel(got[1][k], want[1][k]))


@pytest.mark.parametrize("how", ["plain", "lora"])
def test_mask2former_layer_fused_with_and_without_skipped_queries(how):
    layer, shapes_arg = pixel_decoder_layer("mask2former")
    if how == "lora":
        make_not_plain(layer.self_attn, how)
    layer.to(DEV)
    hidden, kw, pad = pixel_decoder_call(shapes_arg, DEV)
    want = run_attention(layer, hidden, kw)  # transformers' own forward on the GPU
    assert hf_adapter.replace_hf_msda(layer, fused=True) == 1
    log = []
    with spied_symbols(log), KernelTimer() as kt:
        got = run_attention(layer, hidden, kw)
    if how == "lora":
        assert len(log) == 2 and "msda_fwd_fused_levelref_split" in names(kt), (log, names(kt))
    else:
        assert not log and "msda_fwd_fused_levelref" in names(kt), (log, names(kt))
    assert_same_call(got, want, atol=2e-5, rtol=1e-4, gtol=1e-4)
    # padded positions skipped as queries too: real positions are what they were
    assert hf_adapter.replace_hf_msda(layer, fused=True, skip_padded_queries=True) == 0 and layer.self_attn.skip_padded_queries
    out = layer(hidden, **kw)[0].detach().float()
    real = ~pad.to(DEV)
    torch.testing.assert_close(out[real], got[0][real], atol=2e-5, rtol=1e-4)
