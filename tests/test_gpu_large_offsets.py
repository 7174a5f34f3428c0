"""64-bit addressing past 2 GiB and 4 GiB.  Every kernel gives a (batch, head) plane a 64-bit base computed from `b` and
32-bit offsets inside it; here each tensor of the operator in turn crosses the 2^31- and 2^32-byte marks, and the
slices either side of each mark (tests/large_cases.py computes them from the shapes) are held to the fp64 CPU oracle —
with `torch.equal` on exactly representable inputs — while the rest is checked on the device.  Every call is inside
the library's guards (or, in the last section, exactly at one and refused before a launch).  Run with ``-m gpu``; a
test holds at most 32 GiB of device memory (asserted from its shapes) and frees it before the next one."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as ec
import large_cases as lc
from large_cases import DEV, MODES

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
TENSORS = ("out", "grad_value", "grad_loc", "grad_attn")


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


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _shapes(levels):
    return torch.tensor(levels, dtype=torch.int64, device=DEV)


# =========================================================================================================
# a. value planes past 2^32 through the row stride
# =========================================================================================================
A_LEVELS = [(16, 16), (8, 8)]
A_DIMS = dict(B=4, Q=200, H=2, D=32, P=4)


def _strided_value(dense, stride_bytes):
    """`dense` [B, I, H, D] as a view of a large uninitialised buffer, pixels `stride_bytes` apart."""
    B, I, H, D = dense.shape  # noqa: E741
    es = dense.element_size()
    assert stride_bytes % 16 == 0 and stride_bytes >= H * D * es
    buf = torch.empty(B * I * (stride_bytes // es), dtype=dense.dtype, device=DEV)
    view = buf.as_strided((B, I, H, D), (I * (stride_bytes // es), stride_bytes // es, D, 1))
    view.copy_(dense)
    return view


def _case_a(seed=11):
    d = A_DIMS
    return ec.exact_case(np.random.default_rng(seed), d["B"], d["Q"], d["H"], d["D"], A_LEVELS, d["P"])


A_ROUTES = {  # name: (options, what last_launch_info must say)
    "threads256": (dict(lds_levels=0, unit_fwd=0), dict(fwd_variant=0)),
    "lds_one_plane": (dict(lds_levels=2, lds_planes=1, unit_fwd=0), dict(fwd_variant=1, fwd_lds_planes=1)),
    "lds_two_planes": (dict(lds_levels=2, lds_planes=2, unit_fwd=0), dict(fwd_variant=1, fwd_lds_planes=2)),
    "wave_per_unit": (dict(unit_fwd=2), dict(fwd_variant=2)),
}


@pytest.mark.parametrize("vdt", [F32, BF16], ids=["f32", "f32_vbf16"])
def test_value_planes_past_4gib_by_row_stride(vdt):
    """I * stride just under 2^31, B = 4: the planes of batch elements 2 and 3 start just under 2^32 and beyond it.
    Forward by every route, full backward, through the Python API and straight through the C ABI; every batch element
    against the oracle."""
    from msda_triton_amd import _lib, multiscale_deformable_attention
    c = _case_a()
    B, I, H, D = c["value"].shape  # noqa: E741
    Q, L, P = A_DIMS["Q"], len(A_LEVELS), A_DIMS["P"]
    stride = ((1 << 31) - 1) // I // 16 * 16
    assert I * stride < 1 << 31 <= I * (stride + 16) and (B - 1) * I * stride > 1 << 32 > (B - 2) * I * stride
    lc.claim_memory(B * I * stride + (64 << 20), "value planes by row stride")
    value = _strided_value(torch.from_numpy(c["value"]).to(DEV, vdt), stride)
    shapes = _shapes(A_LEVELS)
    loc, attn, go = (torch.from_numpy(c[k]).to(DEV, F32) for k in ("loc", "attn", "grad_out"))
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    suffix, ves = ("f32", 4) if vdt == F32 else ("f32_vbf16", 2)
    for pm, ac in MODES:
        r64 = ec._oracle_all(ec._oracle(), c, pm, ac, np.float64)
        r32 = ec._oracle_all(ec._oracle(), c, pm, ac, np.float32)
        exact = all(np.array_equal(r32[k].astype(np.float64), r64[k]) for k in TENSORS)
        assert exact, "the fixture is not exact in float32"
        for route, (opts, info) in A_ROUTES.items():
            with options(**opts):
                v, l, a = value.detach().requires_grad_(), loc.detach().requires_grad_(), attn.detach().requires_grad_()
                out = multiscale_deformable_attention(v, shapes, l, a, pm, ac)
                got_info = launch_info()
                out.backward(go)
                torch.cuda.synchronize()
            assert {k: got_info[k] for k in info} == info, (route, got_info)
            for k, t in zip(TENSORS, (out, v.grad, l.grad, a.grad)):
                lc.assert_matches(t, r64[k], True, f"{route} {pm} {ac} {k}", forward=k == "out")
        # the C ABI with value_row_stride
        out, gv = torch.empty(B, Q, H, D, device=DEV), torch.empty(B, I, H, D, device=DEV, dtype=vdt)
        gl, ga = torch.empty_like(loc), torch.empty_like(attn)
        ws_bytes = lib.msda_bwd_workspace_bytes(B, I, H, D, Q, L, P, 4, ves, 0, 0)
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=DEV)
        code = _lib.PADDING_MODES[pm]
        assert getattr(lib, f"msda_fwd_{suffix}")(value.data_ptr(), shapes.data_ptr(), loc.data_ptr(), attn.data_ptr(),
                                                  out.data_ptr(), B, I, H, D, Q, L, P, code, int(ac), stride, st) == 0
        assert getattr(lib, f"msda_bwd_{suffix}")(go.data_ptr(), value.data_ptr(), shapes.data_ptr(), loc.data_ptr(),
                                                  attn.data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), B, I, H, D,
                                                  Q, L, P, code, int(ac), 0, stride, ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.synchronize()
        for k, t in zip(TENSORS, (out, gv, gl, ga)):
            lc.assert_matches(t, r64[k], True, f"C ABI {pm} {ac} {k}", forward=k == "out")


def test_value_planes_past_4gib_discrete_sampling():
    from msda_triton_amd import multiscale_deformable_attention
    from test_discrete_sampling import ref_discrete
    c = _case_a(seed=12)
    B, I, H, D = c["value"].shape  # noqa: E741
    counts = [A_DIMS["P"]] * len(A_LEVELS)
    stride = ((1 << 31) - 1) // I // 16 * 16
    lc.claim_memory(B * I * stride + (64 << 20), "value planes by row stride, discrete")
    value = _strided_value(torch.from_numpy(c["value"]).to(DEV, F32), stride)
    loc = torch.from_numpy(c["loc"]).to(DEV, F32).reshape(B, -1, H, sum(counts), 2)
    attn = torch.from_numpy(c["attn"]).to(DEV, F32).reshape(B, -1, H, sum(counts))
    go = torch.from_numpy(c["grad_out"]).to(DEV, F32)
    v, a = value.detach().requires_grad_(), attn.detach().requires_grad_()
    out = multiscale_deformable_attention(v, _shapes(A_LEVELS), loc, a, "border", False, points_per_level=counts,
                                          sampling_mode="discrete")
    assert launch_info()["fwd_variant"] == 3
    out.backward(go)
    torch.cuda.synchronize()
    rv = torch.from_numpy(c["value"]).requires_grad_()
    ra = attn.detach().cpu().double().requires_grad_()
    want = ref_discrete(rv, A_LEVELS, loc.cpu(), ra, counts)
    want.backward(go.cpu().double())
    for k, got, ref in (("out", out, want.detach()), ("grad_value", v.grad, rv.grad), ("grad_attn", a.grad, ra.grad)):
        assert torch.equal(got.cpu().double(), ref), k  # (small integers times dyadic weights: exact in float32)


# =========================================================================================================
# b. one descriptor over the whole tensor (two units per wave) and its fall-back at 2^31 bytes
# =========================================================================================================
@pytest.mark.parametrize("side", ["under", "over"])
def test_two_units_per_wave_switch_at_2gib(side):
    """"unit_waves" 2 serves two units per wave through ONE descriptor over the whole `value` tensor while B * I *
    stride < 2^31 and must fall back to one unit per wave (a descriptor per plane) from 2^31 bytes on.  Two calls that
    differ by 16 bytes of stride, both against the oracle.  (msda_last_launch_info reports "one wave per unit" for
    both kernels: which of the two ran is not observable from outside.)"""
    from msda_triton_amd import multiscale_deformable_attention
    c = ec.exact_case(np.random.default_rng(21), 2, 150, 2, 32, A_LEVELS, 4)
    B, I, H, D = c["value"].shape  # noqa: E741
    under = ((1 << 31) - 1) // (B * I) // 16 * 16
    stride = under if side == "under" else under + 16
    assert B * I * under < 1 << 31 <= B * I * (under + 16) and I * (under + 16) < 1 << 31
    lc.claim_memory(B * I * stride + (64 << 20), "two units per wave")
    value = _strided_value(torch.from_numpy(c["value"]).to(DEV, F32), stride)
    loc, attn = (torch.from_numpy(c[k]).to(DEV, F32) for k in ("loc", "attn"))
    for pm, ac in MODES:
        with options(unit_fwd=2, unit_waves=2):
            out = multiscale_deformable_attention(value, _shapes(A_LEVELS), loc, attn, pm, ac)
            assert launch_info()["fwd_variant"] == 2
        r64 = ec._oracle().forward(c["value"], c["shapes"], c["loc"], c["attn"], pm, ac)
        r32 = ec._oracle().forward(c["value"].astype(np.float32), c["shapes"], c["loc"].astype(np.float32),
                                   c["attn"].astype(np.float32), pm, ac)
        assert np.array_equal(r32.astype(np.float64), r64)
        lc.assert_matches(out, r64, True, f"{side} {pm} {ac}", forward=True)


# =========================================================================================================
# c. sampling tensors past 2^32 bytes
# =========================================================================================================
C_LEVELS = [(8, 8), (4, 4)]
C = dict(B=5, Q=3_400_000, H=2, D=4, S=16)


def _check_sample_slices(picked, value, levels, loc, attn, go, got, pm, ac, counts, what):
    """out / grad_loc / grad_attn of the picked (b, q) slices against the oracle; only those slices leave the device."""
    n_exact = 0
    for b, qs in picked.items():
        q = torch.tensor(qs, device=DEV)
        ref, exact = lc.reference(value[b:b + 1], levels, loc[b:b + 1, q], attn[b:b + 1, q], go[b:b + 1, q], pm, ac, counts)
        n_exact += exact
        for k in ("out", "grad_loc", "grad_attn"):
            lc.assert_matches(got[k][b:b + 1, q], ref[k], exact, f"{what} {pm} {ac} b={b} {k}", forward=k == "out")
    assert n_exact == len(picked), f"{what}: only {n_exact} of {len(picked)} compared slices were exact"


@pytest.mark.parametrize("layout", ["uniform", "points_per_level"])
def test_sampling_tensors_past_4gib(layout):
    """loc and grad_loc (4.35e9 bytes) cross 2^31 and 2^32, attn and grad_attn (2.18e9) cross 2^31; `value` needs no
    gradient, so there is no record workspace."""
    from msda_triton_amd import multiscale_deformable_attention
    B, Q, H, D, S = (C[k] for k in "BQHDS")
    counts = None if layout == "uniform" else [5, 11]
    pts = (len(C_LEVELS), S // len(C_LEVELS)) if counts is None else (S,)
    assert B * Q * H * S * 8 > 1 << 32 and B * Q * H * S * 4 > 1 << 31 and Q * H * S * 2 < 1 << 31
    picked = lc.queries_at_marks(B, Q, {"loc": (H * S * 8, lc.MARKS), "attn": (H * S * 4, lc.MARKS[:1])}, layout)
    units = B * Q * H
    lc.claim_memory(2 * units * S * 12 + 2 * units * D * 4 + units * S * 8 + (1 << 30), f"sampling tensors, {layout}")
    gen = lc.generator(31)
    I = sum(h * w for h, w in C_LEVELS)  # noqa: E741
    value = lc.dev_grid((B, I, H, D), 3, 0, gen)
    loc = lc.dev_odd_multiples((B, Q, H) + pts + (2,), 7, -0.3, 1.3, gen, chunks=B)
    attn = lc.dev_weights((B, Q, H) + pts, 2, gen, chunks=B)
    go = lc.dev_grid((B, Q, H, D), 3, 0, gen, chunks=B)
    kw = {} if counts is None else dict(points_per_level=counts)
    for pm, ac in MODES:
        l, a = loc.detach().requires_grad_(), attn.detach().requires_grad_()
        out = multiscale_deformable_attention(value, _shapes(C_LEVELS), l, a, pm, ac, **kw)
        out.backward(go)
        torch.cuda.synchronize()
        got = dict(out=out.detach(), grad_loc=l.grad, grad_attn=a.grad)
        for k, t in got.items():
            assert bool(torch.isfinite(t).all()), (layout, pm, ac, k)
        _check_sample_slices(picked, value, C_LEVELS, loc, attn, go, got, pm, ac, counts, layout)
        del out, got, l, a


def test_fused_projection_past_4gib():
    """The module's fused core: proj and grad_proj [B, Q, H, L, P, 3] of 6.5e9 bytes cross 2^31 and 2^32 (its guard is
    Q * H * S * 3 < 2^31 per batch element).  The softmax is not exact in float32, so the compared slices take the
    parity file's float32 tolerances; the offsets are dyadic, so no sample sits on a pixel boundary."""
    from msda_triton_amd.functional import fused_module_core, module_sampling_inputs
    B, Q, H, D, S = (C[k] for k in "BQHDS")
    L, P = len(C_LEVELS), S // len(C_LEVELS)
    assert B * Q * H * S * 12 > 1 << 32 and Q * H * S * 3 < 1 << 31
    picked = lc.queries_at_marks(B, Q, {"proj": (H * S * 12, lc.MARKS)}, "fused")
    units = B * Q * H
    lc.claim_memory(2 * units * S * 12 + units * S * 8 + 2 * units * D * 4 + (1 << 30), "fused projection")
    gen = lc.generator(35)
    I = sum(h * w for h, w in C_LEVELS)  # noqa: E741
    value = lc.dev_grid((B, I, H, D), 3, 0, gen)
    proj = torch.empty(B, Q, H, L, P, 3, device=DEV)
    for b in range(B):
        proj[b, ..., :2] = lc.dev_odd_multiples((Q, H, L, P, 2), 4, -3.0, 3.0, gen)
        proj[b, ..., 2] = lc.dev_grid((Q, H, L, P), 2, 0, gen)
    ref = lc.dev_weights((B, Q, 2), 3, gen)
    go = lc.dev_grid((B, Q, H, D), 3, 0, gen, chunks=B)
    shapes = _shapes(C_LEVELS)
    for pm, ac in MODES:
        pr, rf = proj.detach().requires_grad_(), ref.detach().requires_grad_()
        out = fused_module_core(value, shapes, pr, rf, pm, ac)
        out.backward(go)
        torch.cuda.synchronize()
        for k, t in (("out", out), ("grad_proj", pr.grad), ("grad_ref", rf.grad)):
            assert bool(torch.isfinite(t).all()), (pm, ac, k)
        for b, qs in picked.items():
            q = torch.tensor(qs, device=DEV)
            p64 = proj[b:b + 1, q].cpu().double().requires_grad_()
            r64 = ref[b:b + 1, q].cpu().double().requires_grad_()
            pts, att = module_sampling_inputs(p64, shapes.cpu().double(), r64)
            want, _ = lc.reference(value[b:b + 1], C_LEVELS, pts, att, go[b:b + 1, q], pm, ac)
            gp, gr = torch.autograd.grad((pts, att), (p64, r64), (torch.from_numpy(want["grad_loc"]),
                                                                    torch.from_numpy(want["grad_attn"])))
            lc.assert_matches(out[b:b + 1, q], want["out"], False, f"fused {pm} {ac} b={b} out", forward=True)
            lc.assert_matches(pr.grad[b:b + 1, q], gp.numpy(), False, f"fused {pm} {ac} b={b} grad_proj")
            lc.assert_matches(rf.grad[b:b + 1, q], gr.numpy(), False, f"fused {pm} {ac} b={b} grad_ref")
        del out, pr, rf


# =========================================================================================================
# d. row tensors past 2^32: out / grad_out, and grad_value
# =========================================================================================================
D1_LEVELS = [(8, 8), (4, 4)]
D1 = dict(B=8200, Q=2048, H=2, D=32, P=1)


@pytest.mark.parametrize("value_path", [2, 3])
def test_out_and_grad_out_past_4gib(value_path):
    """out and grad_out (4.30e9 bytes each) cross 2^31 and 2^32.  grad_out is zero except at a few hundred queries — the
    ones at the marks and the ends among them, every head of each — so grad_value has an exact reference from those
    queries alone and every other gradient must be zero."""
    from msda_triton_amd import multiscale_deformable_attention
    B, Q, H, D, P = (D1[k] for k in "BQHDP")
    L, I = len(D1_LEVELS), sum(h * w for h, w in D1_LEVELS)  # noqa: E741
    assert B * Q * H * D * 4 > 1 << 32 and Q * H * D * 4 < 1 << 31
    at_marks = lc.mark_slices(B * Q, H * D * 4, lc.MARKS, "out")
    rng = np.random.default_rng(41)
    chosen = sorted(set(at_marks) | {int(g) for g in rng.integers(0, B * Q, size=300)})
    picked = {}
    for g in chosen:
        picked.setdefault(g // Q, []).append(g % Q)
    units = B * Q * H
    ws_guess = units * L * P * 16 * 2 + B * H * I * 4 * D * 4 * 2
    lc.claim_memory(2 * units * D * 4 + 2 * units * L * P * 12 + ws_guess + (1 << 30), "out / grad_out")
    gen = lc.generator(42)
    value = lc.dev_grid((B, I, H, D), 3, 0, gen)
    loc = lc.dev_odd_multiples((B, Q, H, L, P, 2), 7, -0.3, 1.3, gen)
    attn = lc.dev_weights((B, Q, H, L, P), 2, gen)
    go = torch.zeros(B, Q, H, D, device=DEV)
    bq = torch.tensor(chosen, device=DEV)
    go.view(B * Q, H, D)[bq] = lc.dev_grid((len(chosen), H, D), 3, 0, gen)
    assert bool((go.view(B * Q, H, D)[bq].abs().amax(dim=2) > 0).all())  # every head of every chosen query
    pm, ac = MODES[value_path % 2]
    with options(value_path=value_path):
        v, l, a = value.detach().requires_grad_(), loc.detach().requires_grad_(), attn.detach().requires_grad_()
        out = multiscale_deformable_attention(v, _shapes(D1_LEVELS), l, a, pm, ac, level_shapes=D1_LEVELS)
        out.backward(go)
        torch.cuda.synchronize()
        assert launch_info()["value_path"] == (2 if value_path == 2 else 1)
    got = dict(out=out.detach(), grad_value=v.grad, grad_loc=l.grad, grad_attn=a.grad)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), k
    n_exact = 0
    for b, qs in picked.items():
        q = torch.tensor(qs, device=DEV)
        ref, exact = lc.reference(value[b:b + 1], D1_LEVELS, loc[b:b + 1, q], attn[b:b + 1, q], go[b:b + 1, q], pm, ac)
        n_exact += exact
        for k in ("out", "grad_loc", "grad_attn"):
            lc.assert_matches(got[k][b:b + 1, q], ref[k], exact, f"b={b} {k}", forward=k == "out")
        lc.assert_matches(got["grad_value"][b:b + 1], ref["grad_value"], exact, f"b={b} grad_value")
    assert n_exact == len(picked)
    # everything else is zero: batch elements without a chosen query, and the sample gradients of every other query
    others = torch.ones(B, dtype=torch.bool, device=DEV)
    others[torch.tensor(sorted(picked), device=DEV)] = False
    assert not bool(got["grad_value"][others].any())
    for k in ("grad_loc", "grad_attn"):
        rest = got[k].reshape(B * Q, -1).clone()
        rest[bq] = 0
        assert not bool(rest.any()), k
        del rest


D2_LEVELS = [(64, 64), (32, 32), (16, 16), (8, 8)]
D2_I = sum(h * w for h, w in D2_LEVELS)
# name: (value type, B, options, route, passes)
D2 = {
    "sorted_1_pass": (F32, 3100, dict(value_path=2, ws_passes=1), 2, 1),
    "sorted_2_passes": (F32, 3100, dict(value_path=2, ws_passes=2), 2, 2),
    "single_launch": (F32, 3100, dict(value_path=3), 1, 1),
    "single_launch_bf16": (BF16, 6200, dict(value_path=3), 1, 1),
}


@pytest.mark.parametrize("name", list(D2))
def test_grad_value_past_4gib(name):
    """Dense value and grad_value of more than 2^32 bytes (a batch element: 1.4 MB in fp32), two dozen queries per batch
    element.  The batch elements at the 2^31 and 2^32 marks, the first and the last against the oracle; every other one
    on the device: finite, and zero in every row that no sample of that batch element touches."""
    from msda_triton_amd import multiscale_deformable_attention
    vdt, B, opts, route, passes = D2[name]
    Q, H, D, L, P, I = 24, 2, 32, len(D2_LEVELS), 2, D2_I  # noqa: E741
    es = 2 if vdt == BF16 else 4
    plane = I * H * D * es
    assert B * plane > 1 << 32 and plane < 1 << 31
    compared = lc.mark_slices(B, plane, lc.MARKS, "grad_value")
    scratch = B * H * I * 4 * D * 4 // passes if route == 2 else 0  # four partial rows per pixel and plane
    tables = 3 * B * H * (2 * I + 2 * L) * 4 // passes if route == 2 else 0
    lc.claim_memory(2 * B * plane + scratch + tables + (1 << 30), f"grad_value, {name}")
    gen = lc.generator(51)
    value = lc.dev_grid((B, I, H, D), 3, 0, gen, dtype=vdt, chunks=16)
    loc = lc.dev_odd_multiples((B, Q, H, L, P, 2), 8, -0.1, 1.1, gen)
    attn = lc.dev_weights((B, Q, H, L, P), 2, gen)
    go = lc.dev_grid((B, Q, H, D), 3, 0, gen)
    pm, ac = MODES[len(name) % 2]
    with options(**opts):
        v = value.requires_grad_()
        out = multiscale_deformable_attention(v, _shapes(D2_LEVELS), loc, attn, pm, ac, level_shapes=D2_LEVELS)
        out.backward(go)
        torch.cuda.synchronize()
        info = launch_info()
    assert info["value_path"] == route and info["value_passes"] == passes, info
    gv = v.grad
    assert gv.dtype == vdt and gv.is_contiguous() and gv.numel() * gv.element_size() > 1 << 32
    for b in compared:
        ref, exact = lc.reference(value[b:b + 1].detach().float(), D2_LEVELS, loc[b:b + 1], attn[b:b + 1], go[b:b + 1], pm, ac)
        assert exact, f"batch element {b}: the fixture is not exact in float32"
        lc.assert_matches(gv[b:b + 1], ref["grad_value"], True, f"{name} b={b} grad_value")
        lc.assert_matches(out[b:b + 1], ref["out"], True, f"{name} b={b} out", forward=True)
    touched = lc.touched_rows(loc, D2_LEVELS, ac)
    for part, hit in zip(gv.detach().chunk(16, 0), touched.chunk(16, 0)):
        assert bool(torch.isfinite(part).all())
        assert not bool(part[~hit].any()), "a grad_value row that no sample touches is not zero"
    assert bool((gv.detach().abs().amax(dim=(1, 2, 3)) > 0).all())  # ... and every batch element got its gradient


# =========================================================================================================
# e. the guards through the Python API
# =========================================================================================================
def _tiny_call_is_right():
    from msda_triton_amd import multiscale_deformable_attention
    c = ec.exact_case(np.random.default_rng(61), 2, 9, 2, 8, [(4, 4), (2, 3)], 2)
    value, loc, attn = (torch.from_numpy(c[k]).to(DEV, F32) for k in ("value", "loc", "attn"))
    out = multiscale_deformable_attention(value, _shapes([(4, 4), (2, 3)]), loc, attn, "zeros", False)
    torch.cuda.synchronize()
    want = ec._oracle().forward(c["value"], c["shapes"], c["loc"], c["attn"], "zeros", False)
    np.testing.assert_allclose(out.cpu().double().numpy(), want, **lc.FWD_TOL)


@pytest.mark.parametrize("family", ["plain", "ragged", "discrete", "fused"])
def test_python_api_refuses_at_the_limit_and_the_stream_stays_usable(family):
    """Q * H * S * 2 = 2^31 (Q * H * S * 3 >= 2^31 for the fused core): the wrapper raises with the library's message,
    nothing was launched, and the next call on the stream is right.  The tensors are uninitialised (12 GiB at most)."""
    from msda_triton_amd import multiscale_deformable_attention
    from msda_triton_amd.functional import fused_module_core
    levels = [(4, 4), (2, 2)]
    value = torch.zeros(1, 20, 1, 4, device=DEV)
    if family == "fused":
        Q, H, P = 5_600_000, 8, 8
        assert Q * H * 2 * P * 3 >= 1 << 31 > Q * H * 2 * P * 2
        lc.claim_memory(Q * H * 2 * P * 12 + (1 << 30), "guard, fused")
        value = torch.zeros(1, 20, H, 4, device=DEV)
        proj = torch.empty(1, Q, H, 2, P, 3, device=DEV)
        ref = torch.empty(1, Q, 2, device=DEV)
        with pytest.raises(ValueError, match="too large"):
            fused_module_core(value, _shapes(levels), proj, ref, "zeros", False)
        del proj, ref
    else:
        Q, S = 1 << 10, 1 << 20
        lc.claim_memory(Q * S * 12 + (1 << 30), f"guard, {family}")
        if family == "plain":
            loc, attn, kw = torch.empty(1, Q, 1, 2, S // 2, 2, device=DEV), torch.empty(1, Q, 1, 2, S // 2, device=DEV), {}
        else:
            loc, attn = torch.empty(1, Q, 1, S, 2, device=DEV), torch.empty(1, Q, 1, S, device=DEV)
            kw = dict(points_per_level=[S // 2, S // 2])
            if family == "discrete":
                kw["sampling_mode"] = "discrete"
        with pytest.raises(ValueError, match="too large"):
            multiscale_deformable_attention(value, _shapes(levels), loc, attn, "border", False, **kw)
        del loc, attn
    _tiny_call_is_right()


def test_python_api_copies_a_view_whose_plane_stride_reaches_2gib():
    """A strided `value` view with I * stride >= 2^31 is not addressable in place: the wrapper reads a dense copy (what
    functional._value_rows and the binding's value_rows document), and the result is right."""
    from msda_triton_amd import functional, multiscale_deformable_attention
    c = ec.exact_case(np.random.default_rng(71), 1, 50, 2, 32, A_LEVELS, 4)
    I = c["value"].shape[1]  # noqa: E741
    stride = ((1 << 31) // I // 16 + 1) * 16
    assert I * stride >= 1 << 31 > I * (stride - 16)
    lc.claim_memory(I * stride + (64 << 20), "a view beyond the plane stride")
    value = _strided_value(torch.from_numpy(c["value"]).to(DEV, F32), stride)
    dense, row = functional._value_rows(value)
    assert row == 0 and dense.is_contiguous()
    loc, attn, go = (torch.from_numpy(c[k]).to(DEV, F32) for k in ("loc", "attn", "grad_out"))
    for pm, ac in MODES:
        v, l, a = value.detach().requires_grad_(), loc.detach().requires_grad_(), attn.detach().requires_grad_()
        out = multiscale_deformable_attention(v, _shapes(A_LEVELS), l, a, pm, ac)
        out.backward(go)
        torch.cuda.synchronize()
        r64 = ec._oracle_all(ec._oracle(), c, pm, ac, np.float64)
        for k, t in zip(TENSORS, (out, v.grad, l.grad, a.grad)):
            lc.assert_matches(t, r64[k], True, f"{pm} {ac} {k}", forward=k == "out")
