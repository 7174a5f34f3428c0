"""GPU: what the fused launchers of msda_triton_amd.functional / .ragged / .discrete send across the C ABI.

The expected argument lists below are written from include/msda_hip.h, slot by slot, not from the launchers.  Each test
replaces the ctypes function on the loaded handle (and the workspace-size query the backward uses) with a recorder that
stores its arguments and forwards to the real function, so every recorded call is a valid call that runs.  Held per
family and direction: the symbol, every scalar, the contents of the counts and level-scale arrays, every pointer (inputs
by identity with the tensors passed in, outputs by identity with what the launcher returns), the query's own arguments —
the arithmetic element size in particular: 4 under a storage suffix, the projection's otherwise —, ``workspace_bytes``
equal to the query's answer, and a null ``grad_value`` / workspace for a frozen pyramid.

Shapes: B=2, Q=3, H=2, D=8, levels (2, 3) and (1, 2); P=2 (and P=3, so that L != P) for the uniform families, counts
(2, 1) for the per-level ones.  "zeros" / align_corners=False so that the two codes differ.

Declined calls (``None``, nothing returned) one sample above ``fused_lp_limit``: `test_declined_one_above_the_limit` here
for the launchers (the backward; the forward's own bound is higher, see there); through the routing functions tests/test_gpu_hf_fused.py, tests/test_gpu_levelref_split.py and
tests/test_gpu_sample_level_sweep.py hold the same.  The two discrete pairs have no sample limit: their launchers decline
more than 8 levels without a call, held here as well."""
import ctypes

import numpy as np
import pytest
import torch

from msda_triton_amd import _lib, discrete, ragged
from msda_triton_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, Q, H, D = 2, 3, 2, 8
LEVELS = ((2, 3), (1, 2))
I, L = sum(h * w for h, w in LEVELS), len(LEVELS)  # noqa: E741
COUNTS = (2, 1)
S = sum(COUNTS)
CELLS = max((h + 1) * (w + 1) for h, w in LEVELS)
PAD, PAD_CODE, AC = "zeros", 1, False
SCALE = 0.3
# (value, projection, reference points) dtypes and the suffix the header gives them
CASES = {"fp32": (torch.float32, torch.float32, torch.float32, "f32"),
         "sbf16": (torch.bfloat16, torch.bfloat16, torch.float32, "f32_sbf16")}
ROW_PAD = 64  # bytes behind a pixel's H * D channels in the padded case


class Recorder:
    """stores (arguments, result) of every call and forwards to the real entry point"""

    def __init__(self, real, before=None):
        self.real, self.calls, self.before = real, [], before

    def __call__(self, *args):
        if self.before is not None:
            self.before(args)
        res = self.real(*args)
        self.calls.append((args, res))
        return res


def spy(monkeypatch, symbol, before=None):
    lib = _lib.load()
    rec = Recorder(getattr(lib, symbol), before)
    monkeypatch.setattr(lib, symbol, rec)
    return rec


# ---------------------------------------------------------------------------------------- one expected slot each
def ptr(t):
    return ("ptr", t)


def num(v):
    return ("num", v)


NULL, SOME, STREAM = ("null", None), ("some", None), ("stream", None)


def assert_slots(args, spec, what):
    assert len(args) == len(spec), f"{what}: {len(args)} arguments, the header declares {len(spec)}"
    seen = []
    for i, (got, (kind, want)) in enumerate(zip(args, spec)):
        where = f"{what}: argument {i}"
        if kind == "ptr":
            assert got == want.data_ptr(), where
            seen.append(got)
        elif kind == "null":
            assert got is None or got == 0, where
        elif kind == "some":  # (a buffer the launcher keeps to itself: non-null and no other slot's)
            assert got and got not in seen, where
            seen.append(got)
        elif kind == "num":
            assert isinstance(got, type(want)) and got == want, f"{where}: {got!r}, expected {want!r}"
        elif kind == "counts":
            assert got._type_ is ctypes.c_int32 and list(got) == list(want), where
        elif kind == "scales":
            assert got._type_ is ctypes.c_float and list(got) == [float(np.float32(1 / p)) for p in want], where
        elif kind == "stream":
            assert (got or 0) == torch.cuda.current_stream(torch.device(DEV)).cuda_stream, where


def dims(P=None):
    """B, I, H, D, Q, L and then P or the host array of counts"""
    return [num(B), num(I), num(H), num(D), num(Q), num(L), num(P) if P is not None else ("counts", COUNTS)]


def check_forward(rec, lead, extras, tail, out, P=None):
    """value, <lead>, out, dims, <extras>, <tail>, stream"""
    (args, rc), = rec.calls
    assert rc == 0 and out is not None
    assert_slots(args, lead + [ptr(out)] + dims(P) + extras + tail + [STREAM], "forward")
    assert tuple(out.shape) == (B, Q, H, D) and out.is_contiguous()


def check_backward(rec, query, lead, grads, extras, tail, value, elem, need_img, P=None):
    """grad_out, value, <lead>, grad_value, <grads>, dims, <extras>, <tail>, workspace, workspace_bytes, stream; and the
    size query: dims, elem_size, value_elem_size, max_level_cells, flags"""
    (args, rc), = rec.calls
    assert rc == 0
    if need_img:
        (qargs, ws_bytes), = query.calls
        assert_slots(qargs, dims(P) + [num(elem), num(value.element_size()), num(CELLS), num(0)], "size query")
        assert ws_bytes > 0
        ws = [SOME, num(ws_bytes)]
    else:
        assert query.calls == []
        ws = [NULL, num(0)]
    assert_slots(args, lead + grads + dims(P) + extras + tail + ws + [STREAM], "backward")


# ---------------------------------------------------------------------------------------- inputs
def make(case, sample_shape, ref_shape, padded=False, seed=1):
    vdt, pdt, rdt, _ = CASES[case]
    g = torch.Generator(device="cpu").manual_seed(seed)
    value = torch.randn(B, I, H, D, generator=g).to(vdt).to(DEV)
    if padded:
        rows = F.padded_value_rows(B, I, H, D, vdt, DEV, pad_bytes=ROW_PAD)
        rows.copy_(value)
        value = rows
    shapes = torch.tensor(LEVELS, dtype=torch.int64, device=DEV)
    proj = (torch.randn(B, Q, H, *sample_shape, 3, generator=g) * 1.5).to(pdt).to(DEV)
    ref = (torch.rand(B, Q, *ref_shape, generator=g) * 0.5 + 0.25).to(rdt).to(DEV)
    gout = torch.rand(B, Q, H, D, generator=g).to(pdt).to(DEV)
    return value, shapes, proj, ref, gout


def masks(which):
    """contiguous uint8 masks with one padding pixel / one padded query: the launchers pass them on as they are"""
    vm = torch.ones(B, I, dtype=torch.uint8, device=DEV)
    vm[1, I - 1] = 0
    qm = torch.ones(B, Q, dtype=torch.uint8, device=DEV)
    qm[0, Q - 1] = 0
    return {"": (None, None), "value": (vm, None), "both": (vm, qm)}[which]


def stride_of(padded, value):
    return H * D * value.element_size() + ROW_PAD if padded else 0


def elem_of(case, proj):
    return 4 if case == "sbf16" else proj.element_size()


SAMPLING_TAIL = [num(PAD_CODE), num(int(AC))]


# ---------------------------------------------------------------------------------------- module and level-reference pairs
# name -> (infix, levelref, masks given, mask pointers in the list: the module's masked pair takes both, always)
UNIFORM = {"module": ("fused", False, "", 0), "module_masked": ("fused_masked", False, "both", 2),
           "levelref": ("fused_levelref", True, "", 0), "levelref_masked": ("fused_levelref_masked", True, "value", 1),
           "levelref_qmasked": ("fused_levelref_qmasked", True, "both", 2)}


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("case,padded,need_img", [("fp32", False, True), ("sbf16", False, True), ("fp32", True, True),
                                                  ("fp32", False, False)],
                         ids=["fp32", "sbf16", "padded", "frozen"])
@pytest.mark.parametrize("family", list(UNIFORM))
def test_uniform_pairs(monkeypatch, family, case, padded, need_img, ref_dim, P):
    infix, levelref, which, nmask = UNIFORM[family]
    suf = CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (L, P), (L, ref_dim) if levelref else (ref_dim,), padded)
    vm, qm = masks(which)
    mask_slots = [ptr(vm), ptr(qm)][:nmask]
    vrow = stride_of(padded, value)
    fwd = spy(monkeypatch, f"msda_fwd_{infix}_{suf}")
    out = F.msda_hip_fwd_fused(value, shapes, proj, ref, PAD, AC, levelref=levelref, value_mask=vm, query_mask=qm)
    check_forward(fwd, [ptr(value)] + mask_slots + [ptr(shapes), ptr(proj), ptr(ref)], [num(ref_dim)],
                  SAMPLING_TAIL + [num(vrow)], out, P)
    assert out.dtype == proj.dtype
    bwd, query = spy(monkeypatch, f"msda_bwd_{infix}_{suf}"), spy(monkeypatch, "msda_bwd_fused_workspace_bytes")
    g_img, g_proj, g_ref = F.msda_hip_bwd_fused(gout, value, shapes, proj, ref, PAD, AC, need_img, level_cells=CELLS,
                                                levelref=levelref, value_mask=vm, query_mask=qm)
    check_backward(bwd, query, [ptr(gout), ptr(value)] + mask_slots + [ptr(shapes), ptr(proj), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_proj), SOME], [num(ref_dim)],
                   SAMPLING_TAIL + [num(CELLS), num(vrow)], value, elem_of(case, proj), need_img, P)
    assert (g_img is None) == (not need_img) and (g_img is None or (g_img.shape == value.shape and g_img.dtype == value.dtype))
    assert g_proj.shape == proj.shape and g_proj.dtype == proj.dtype and g_ref.shape == ref.shape and g_ref.dtype == ref.dtype


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("case,padded,need_img", [("fp32", False, True), ("sbf16", False, True), ("fp32", True, True),
                                                  ("fp32", False, False)],
                         ids=["fp32", "sbf16", "padded", "frozen"])
def test_split_pair(monkeypatch, case, padded, need_img, ref_dim, P):
    suf = CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (L, P), (L, ref_dim), padded)
    offsets, logits = proj[..., :2].contiguous(), proj[..., 2].contiguous()
    vrow = stride_of(padded, value)
    fwd = spy(monkeypatch, f"msda_fwd_fused_levelref_split_{suf}")
    out = F.msda_hip_fwd_fused_split(value, shapes, offsets, logits, ref, PAD, AC)
    check_forward(fwd, [ptr(value), ptr(shapes), ptr(offsets), ptr(logits), ptr(ref)], [num(ref_dim)],
                  SAMPLING_TAIL + [num(vrow)], out, P)
    bwd, query = spy(monkeypatch, f"msda_bwd_fused_levelref_split_{suf}"), spy(monkeypatch, "msda_bwd_fused_workspace_bytes")
    g_img, g_off, g_lgt, g_ref = F.msda_hip_bwd_fused_split(gout, value, shapes, offsets, logits, ref, PAD, AC, need_img,
                                                            level_cells=CELLS)
    check_backward(bwd, query, [ptr(gout), ptr(value), ptr(shapes), ptr(offsets), ptr(logits), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_off), ptr(g_lgt), SOME], [num(ref_dim)],
                   SAMPLING_TAIL + [num(CELLS), num(vrow)], value, elem_of(case, offsets), need_img, P)
    assert (g_img is None) == (not need_img)
    assert g_off.shape == offsets.shape and g_lgt.shape == logits.shape and g_ref.shape == ref.shape


# ---------------------------------------------------------------------------------------- the per-level-count pairs
PER_LEVEL_CASES = pytest.mark.parametrize(
    "case,padded,need_img", [("fp32", False, True), ("sbf16", False, True), ("fp32", True, True), ("fp32", False, False)],
    ids=["fp32", "sbf16", "padded", "frozen"])


@pytest.mark.parametrize("ref_dim", [2, 4])
@PER_LEVEL_CASES
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_ragged_pair(monkeypatch, masked, case, padded, need_img, ref_dim):
    infix, suf = ("fused_ragged_masked" if masked else "fused_ragged"), CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (S,), (ref_dim,), padded)
    vm, qm = masks("both" if masked else "")
    mask_slots = [ptr(vm), ptr(qm)] if masked else []
    vrow = stride_of(padded, value)
    fwd = spy(monkeypatch, f"msda_fwd_{infix}_{suf}")
    out = ragged.ragged_hip_fwd_fused(value, shapes, proj, ref, PAD, AC, COUNTS, vm, qm)
    check_forward(fwd, [ptr(value)] + mask_slots + [ptr(shapes), ptr(proj), ptr(ref)], [num(ref_dim)],
                  SAMPLING_TAIL + [num(vrow)], out)
    bwd, query = spy(monkeypatch, f"msda_bwd_{infix}_{suf}"), spy(monkeypatch, "msda_bwd_fused_ragged_workspace_bytes")
    g_img, g_proj, g_ref = ragged.ragged_hip_bwd_fused(gout, value, shapes, proj, ref, PAD, AC, COUNTS, need_img,
                                                       level_cells=CELLS, value_mask=vm, query_mask=qm)
    check_backward(bwd, query, [ptr(gout), ptr(value)] + mask_slots + [ptr(shapes), ptr(proj), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_proj), SOME], [num(ref_dim)],
                   SAMPLING_TAIL + [num(CELLS), num(vrow)], value, elem_of(case, proj), need_img)
    assert (g_img is None) == (not need_img) and g_proj.shape == proj.shape and g_ref.shape == ref.shape


def box_points(proj, ref):
    """the box rule's points and weights in the arithmetic dtype (float32 next to 16-bit storage)"""
    return F.hf_box_sampling_inputs(proj.to(ref.dtype), ref, COUNTS, SCALE)


def assert_parked(case, got_points, want_points, got_weights=None, want_weights=None):
    """float32 / the arithmetic dtype; fp32: the prologue's points bit for bit and the kernel's softmax to rounding, the
    tolerances of tests/test_gpu_hf_box_discrete.py; behind 16-bit storage the points to that rounding too"""
    assert got_points.dtype == torch.float32 and got_points.shape == want_points.shape
    if case == "fp32":
        assert torch.equal(got_points, want_points)
    else:
        torch.testing.assert_close(got_points, want_points, atol=0.0, rtol=1e-5)
    if want_weights is not None:
        assert got_weights.dtype == torch.float32
        torch.testing.assert_close(got_weights, want_weights, atol=0.0, rtol=1e-5)


@PER_LEVEL_CASES
def test_hfbox_pair(monkeypatch, case, padded, need_img):
    suf = CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (S,), (4,), padded)
    vrow = stride_of(padded, value)
    box = [("counts", COUNTS), ("scales", COUNTS), num(SCALE), num(4)]
    fwd = spy(monkeypatch, f"msda_fwd_fused_hfbox_{suf}")
    out = ragged.hf_box_hip_fwd_fused(value, shapes, proj, ref, PAD, AC, COUNTS, SCALE)
    check_forward(fwd, [ptr(value), ptr(shapes), ptr(proj), ptr(ref)], box[1:], SAMPLING_TAIL + [num(vrow)], out)
    bwd, query = spy(monkeypatch, f"msda_bwd_fused_hfbox_{suf}"), spy(monkeypatch, "msda_bwd_fused_ragged_workspace_bytes")
    res = ragged.hf_box_hip_bwd_fused(gout, value, shapes, proj, ref, PAD, AC, COUNTS, SCALE, need_img, level_cells=CELLS,
                                      parked_points=True)
    g_img, g_proj, g_ref = res[:3]
    check_backward(bwd, query, [ptr(gout), ptr(value), ptr(shapes), ptr(proj), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_proj), SOME], box[1:],
                   SAMPLING_TAIL + [num(CELLS), num(vrow)], value, elem_of(case, proj), need_img)
    assert g_proj.shape == proj.shape and g_ref.shape == ref.shape
    assert len(res) == (4 if need_img else 3)  # (the points are parked for grad_value's passes only)
    if need_img:
        assert_parked(case, res[3], box_points(proj, ref)[0])


@PER_LEVEL_CASES
def test_hfbox_discrete_pair(monkeypatch, case, padded, need_img):
    suf = CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (S,), (4,), padded)
    vrow = stride_of(padded, value)
    box = [("scales", COUNTS), num(SCALE)]
    fwd = spy(monkeypatch, f"msda_fwd_fused_hfbox_discrete_{suf}")
    out = discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref, COUNTS, SCALE)
    check_forward(fwd, [ptr(value), ptr(shapes), ptr(proj), ptr(ref)], box, [num(vrow)], out)
    bwd = spy(monkeypatch, f"msda_bwd_fused_hfbox_discrete_{suf}")
    query = spy(monkeypatch, "msda_bwd_fused_hfbox_discrete_workspace_bytes")
    res = discrete.hf_box_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, COUNTS, SCALE, need_img, level_cells=CELLS,
                                                 parked_points=True)
    g_img, g_proj = res[:2]
    check_backward(bwd, query, [ptr(gout), ptr(value), ptr(shapes), ptr(proj), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_proj)], box, [num(CELLS), num(vrow)], value,
                   elem_of(case, proj), need_img)
    assert g_proj.shape == proj.shape and len(res) == (4 if need_img else 2)
    if need_img:
        assert_parked(case, res[2], box_points(proj, ref)[0], res[3], box_points(proj, ref)[1])


@pytest.mark.parametrize("ref_dim", [2, 4])
@PER_LEVEL_CASES
def test_module_discrete_pair(monkeypatch, case, padded, need_img, ref_dim):
    suf = CASES[case][3]
    value, shapes, proj, ref, gout = make(case, (S,), (ref_dim,), padded)
    vrow = stride_of(padded, value)
    fwd = spy(monkeypatch, f"msda_fwd_fused_discrete_{suf}")
    out = discrete.module_discrete_hip_fwd_fused(value, shapes, proj, ref, COUNTS)
    check_forward(fwd, [ptr(value), ptr(shapes), ptr(proj), ptr(ref)], [num(ref_dim)], [num(vrow)], out)
    bwd, query = spy(monkeypatch, f"msda_bwd_fused_discrete_{suf}"), spy(monkeypatch, "msda_bwd_fused_discrete_workspace_bytes")
    res = discrete.module_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, COUNTS, need_img, level_cells=CELLS,
                                                 parked_points=True)
    g_img, g_proj = res[:2]
    check_backward(bwd, query, [ptr(gout), ptr(value), ptr(shapes), ptr(proj), ptr(ref)],
                   [ptr(g_img) if need_img else NULL, ptr(g_proj)], [num(ref_dim)], [num(CELLS), num(vrow)], value,
                   elem_of(case, proj), need_img)
    assert g_proj.shape == proj.shape and len(res) == (4 if need_img else 2)
    if need_img:
        # (the module's rule on host tensors, as tests/test_gpu_module_discrete.py states its yardstick)
        pts, att = ragged.ragged_module_sampling_inputs(proj.cpu().to(ref.dtype), shapes.cpu(), ref.cpu(), COUNTS)
        assert_parked(case, res[2].cpu(), pts, res[3].cpu(), att)


# ---------------------------------------------------------------------------------------- the out_grad rule
def other_out_grad(gout):
    """the same numbers, non-contiguous and in another dtype (float64 holds every float32 / bfloat16 exactly)"""
    wide = torch.empty(B, Q, H, 2 * D, dtype=torch.float64, device=DEV)
    view = wide[..., ::2]
    view.copy_(gout)
    assert not view.is_contiguous() and view.dtype != gout.dtype
    return view


def device_bytes(pointer, nbytes):
    """nbytes of device memory behind a raw pointer, as the library is about to read them"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    buf = ctypes.create_string_buffer(nbytes)
    torch.cuda.synchronize()
    assert hip.hipMemcpy(buf, pointer, nbytes, 2) == 0  # (hipMemcpyDeviceToHost)
    return buf.raw


def backward_of(family, case):
    """-> (symbol, a contiguous out_grad of the compute dtype, call(out_grad) -> gradients); grad_out is slot 0 everywhere"""
    suf = CASES[case][3]
    if family in ("module", "levelref"):
        lr = family == "levelref"
        v, s, p, r, g = make(case, (L, 2), (L, 2) if lr else (2,))
        return f"msda_bwd_fused{'_levelref' if lr else ''}_{suf}", g, \
            lambda og: F.msda_hip_bwd_fused(og, v, s, p, r, PAD, AC, levelref=lr)
    if family == "split":
        v, s, p, r, g = make(case, (L, 2), (L, 2))
        off, lgt = p[..., :2].contiguous(), p[..., 2].contiguous()
        return f"msda_bwd_fused_levelref_split_{suf}", g, lambda og: F.msda_hip_bwd_fused_split(og, v, s, off, lgt, r, PAD, AC)
    if family == "ragged":
        v, s, p, r, g = make(case, (S,), (2,))
        return f"msda_bwd_fused_ragged_{suf}", g, lambda og: ragged.ragged_hip_bwd_fused(og, v, s, p, r, PAD, AC, COUNTS)
    if family == "hfbox":
        v, s, p, r, g = make(case, (S,), (4,))
        return f"msda_bwd_fused_hfbox_{suf}", g, lambda og: ragged.hf_box_hip_bwd_fused(og, v, s, p, r, PAD, AC, COUNTS, SCALE)
    if family == "hfbox_discrete":
        v, s, p, r, g = make(case, (S,), (4,))
        return f"msda_bwd_fused_hfbox_discrete_{suf}", g, \
            lambda og: discrete.hf_box_discrete_hip_bwd_fused(og, v, s, p, r, COUNTS, SCALE)
    v, s, p, r, g = make(case, (S,), (2,))
    return f"msda_bwd_fused_discrete_{suf}", g, lambda og: discrete.module_discrete_hip_bwd_fused(og, v, s, p, r, COUNTS)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("family", ["module", "levelref", "split", "ragged", "hfbox", "hfbox_discrete", "module_discrete"])
def test_out_grad_is_passed_contiguous_in_the_compute_dtype(monkeypatch, family, case):
    symbol, gout, call = backward_of(family, case)
    want = call(gout)
    # what the library is handed as grad_out: B * Q * H * D elements of the compute dtype, dense, the pre-converted numbers
    nbytes, read = gout.numel() * gout.element_size(), []
    rec = spy(monkeypatch, symbol, before=lambda args: read.append(device_bytes(args[0], nbytes)))
    got = call(other_out_grad(gout))
    (args, rc), = rec.calls
    assert rc == 0 and args[0] != gout.data_ptr()
    assert read[0] == gout.cpu().view(torch.uint8).numpy().tobytes()
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b)


# ---------------------------------------------------------------------------------------- declined calls
def test_declined_one_above_the_limit():
    """L * P (sum(counts)) one above msda_fused_lp_limit(D, 4): the backward returns None, no gradient.  The limit is the
    backward's — its LDS records are 16 + 7 * 4 bytes a sample, the forward's 16 + 4 * 4 (msda_launch.hpp, plan_gather), so
    the forward still takes limit + 1 samples (tests/sample_level_cases.py, "_over"); it is held to None at twice that,
    beyond 44 / 32 of the limit."""
    over = F.fused_lp_limit(D, 4) + 1
    far = 2 * over
    levels1 = torch.tensor([LEVELS[0]], dtype=torch.int64, device=DEV)
    n1 = LEVELS[0][0] * LEVELS[0][1]
    g = torch.Generator(device="cpu").manual_seed(3)
    value1 = torch.randn(B, n1, H, D, generator=g).to(DEV)
    gout = torch.rand(B, Q, H, D, generator=g).to(DEV)
    wide = torch.randn(B, Q, H, 1, far, 3, generator=g).to(DEV)
    proj = wide[:, :, :, :, :over].contiguous()
    for levelref in (False, True):
        ref = torch.rand(B, Q, *((1, 2) if levelref else (2,)), generator=g).to(DEV)
        assert F.msda_hip_fwd_fused(value1, levels1, wide, ref, PAD, AC, levelref=levelref) is None
        assert F.msda_hip_bwd_fused(gout, value1, levels1, proj, ref, PAD, AC, levelref=levelref) is None
    ref = torch.rand(B, Q, 1, 2, generator=g).to(DEV)
    assert F.msda_hip_fwd_fused_split(value1, levels1, wide[..., :2].contiguous(), wide[..., 2].contiguous(), ref, PAD,
                                      AC) is None
    assert F.msda_hip_bwd_fused_split(gout, value1, levels1, proj[..., :2].contiguous(), proj[..., 2].contiguous(), ref, PAD,
                                      AC) is None
    # per-level counts: (limit, 1) over the two levels for the backward, (2 * limit + 1, 1) for the forward
    value, shapes, _, _, _ = make("fp32", (S,), (2,))
    wide, proj = wide[:, :, :, 0], proj[:, :, :, 0]
    ref2, ref4 = torch.rand(B, Q, 2, generator=g).to(DEV), torch.rand(B, Q, 4, generator=g).to(DEV)
    assert ragged.ragged_hip_fwd_fused(value, shapes, wide, ref2, PAD, AC, (far - 1, 1)) is None
    assert ragged.ragged_hip_bwd_fused(gout, value, shapes, proj, ref2, PAD, AC, (over - 1, 1)) is None
    assert ragged.hf_box_hip_fwd_fused(value, shapes, wide, ref4, PAD, AC, (far - 1, 1), SCALE) is None
    assert ragged.hf_box_hip_bwd_fused(gout, value, shapes, proj, ref4, PAD, AC, (over - 1, 1), SCALE) is None


def test_discrete_pairs_decline_nine_levels_without_a_call(monkeypatch):
    levels = [(1, 1)] * (discrete.FUSED_BOX_MAX_LEVELS + 1)
    counts = (1,) * len(levels)
    shapes = torch.tensor(levels, dtype=torch.int64, device=DEV)
    value = torch.randn(B, len(levels), H, D, device=DEV)
    proj = torch.randn(B, Q, H, len(levels), 3, device=DEV)
    ref, gout = torch.rand(B, Q, 4, device=DEV), torch.rand(B, Q, H, D, device=DEV)
    recs = [spy(monkeypatch, f"msda_{d}_fused_{f}_f32") for d in ("fwd", "bwd") for f in ("hfbox_discrete", "discrete")]
    assert discrete.hf_box_discrete_hip_fwd_fused(value, shapes, proj, ref, counts, SCALE) is None
    assert discrete.hf_box_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, counts, SCALE) is None
    assert discrete.module_discrete_hip_fwd_fused(value, shapes, proj, ref, counts) is None
    assert discrete.module_discrete_hip_bwd_fused(gout, value, shapes, proj, ref, counts) is None
    assert all(r.calls == [] for r in recs)
