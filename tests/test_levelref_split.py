"""The per-level-reference fused pair on SPLIT projections (msda_*_fused_levelref_split_<suffix>), without a GPU: the
symbols, the header's macro, the ctypes lists against the interleaved pair's, the argument-error table on host addresses,
the host definition of ``fused_hf_module_core_split``, and the Hugging Face adapter behind projection layers that are not
plain ``nn.Linear`` (a LoRA-like subclass, a forward hook) and on Mask2Former's / OneFormer's pixel-decoder modules.

Tolerances: the adapter tests use what tests/test_hf_fused.py uses on the host — ``atol=1e-5, rtol=1e-4`` for outputs, a
relative L2 error below 1e-4 per gradient tensor.  The host definition is an equality (``torch.equal``)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from msda_triton_amd import _lib, _linear
from msda_triton_amd.functional import (fused_hf_module_core, fused_hf_module_core_split, split_projection_views,
                                        stack_split_projection)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUFFIXES = _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES
# (arithmetic / reference points, value rows, projection and out) element sizes per suffix
SIZES = {"f32": (4, 4, 4), "f16": (2, 2, 2), "bf16": (2, 2, 2), "f64": (8, 8, 8), "f32_vbf16": (4, 2, 4),
         "f32_vf16": (4, 2, 4), "f32_sbf16": (4, 2, 2), "f32_sf16": (4, 2, 2)}
BAD_ARG, TOO_MANY_LEVELS, TOO_LARGE, MISALIGNED, UNSUPPORTED = -1, -2, -3, -4, -5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ symbols and lists
def test_the_symbol_table(lib):
    assert _lib.has_levelref_split()
    want = {f"msda_{d}_fused_levelref_split_{s}" for d in ("fwd", "bwd") for s in SUFFIXES}
    assert len(_lib.LEVELREF_SPLIT_SYMBOLS) == 16 and set(_lib.LEVELREF_SPLIT_SYMBOLS) == want
    for other in (_lib.EXPORTED_SYMBOLS, _lib.QUERY_MASK_SYMBOLS, _lib.HFBOX_DISCRETE_SYMBOLS, _lib.MODULE_MASK_SYMBOLS,
                  _lib.MODULE_DISCRETE_SYMBOLS):
        assert not set(_lib.LEVELREF_SPLIT_SYMBOLS) & set(other)
    for s in _lib.LEVELREF_SPLIT_SYMBOLS:
        assert hasattr(lib, s), s
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(_lib.LEVELREF_SPLIT_SYMBOLS) <= set(re.findall(r" T (msda_\w+)", nm))
    assert lib.msda_abi_version() == 12


def _macro_decls(text, macro):
    body = re.search(r"#define " + macro + r"\(SUF\)(.*)", text).group(1)
    return {name: [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
            for name, params in re.findall(r"int msda_(\w+)_##SUF\(([^)]*)\)", body)}


def test_the_header_declares_them_through_a_macro_of_its_own():
    with open(os.path.join(ROOT, "include", "msda_hip.h")) as f:
        text = f.read().replace("\\\n", " ")
    decl = _macro_decls(text, "MSDA_LEVELREF_SPLIT")
    assert set(decl) == {"fwd_fused_levelref_split", "bwd_fused_levelref_split"}
    used = re.findall(r"MSDA_LEVELREF_SPLIT\((\w+)\)", text)
    assert sorted(s for s in used if s != "SUF") == sorted(SUFFIXES)
    assert "#undef MSDA_LEVELREF_SPLIT\n" in text
    twins = {}
    for name, body in re.findall(r"#define (MSDA_DECLARE\w*)\(SUF\)(.*)", text):  # (those macros are EXPORTED_SYMBOLS')
        assert "levelref_split_##SUF" not in body, name
        twins.update(_macro_decls(text, name))
    fwd, bwd = twins["fwd_fused_levelref"], twins["bwd_fused_levelref"]
    at = fwd.index("const void *proj")
    assert decl["fwd_fused_levelref_split"] == fwd[:at] + ["const void *offsets", "const void *logits"] + fwd[at + 1:]
    at, gat = bwd.index("const void *proj"), bwd.index("void *grad_proj")
    assert decl["bwd_fused_levelref_split"] == (bwd[:at] + ["const void *offsets", "const void *logits"] + bwd[at + 1:gat]
                                                + ["void *grad_offsets", "void *grad_logits"] + bwd[gat + 1:])


def test_each_ctypes_list_is_the_twins_with_one_more_pointer_per_projection(lib):
    vp = ctypes.c_void_p
    for s in SUFFIXES:
        mine, twin = getattr(lib, f"msda_fwd_fused_levelref_split_{s}"), getattr(lib, f"msda_fwd_fused_levelref_{s}")
        assert list(mine.argtypes) == [vp] + list(twin.argtypes) and mine.restype is ctypes.c_int
        assert list(twin.argtypes[:5]) == [vp] * 5
        mine, twin = getattr(lib, f"msda_bwd_fused_levelref_split_{s}"), getattr(lib, f"msda_bwd_fused_levelref_{s}")
        assert list(mine.argtypes) == [vp, vp] + list(twin.argtypes) and mine.restype is ctypes.c_int
        assert list(twin.argtypes[:8]) == [vp] * 8


# ---------------------------------------------------------------------------------------------- argument-error table
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the rows pass host addresses as buffers: safe only where a "
                            "call that slipped past its guard cannot launch (the GPU side: test_gpu_levelref_split.py)")
DIMS = dict(B=1, I=4, H=1, D=4, Q=1, L=1, P=1)
BUFFERS = ("grad_out", "value", "shapes", "offsets", "logits", "ref", "out", "grad_value", "grad_offsets", "grad_logits",
           "grad_ref")


def _spec(direction, split=True):
    proj = ["offsets", "logits"] if split else ["offsets"]
    gproj = ["grad_offsets", "grad_logits"] if split else ["grad_offsets"]
    names = (["grad_out"] if direction == "bwd" else []) + ["value", "shapes"] + proj + ["ref"]
    names += ["out"] if direction == "fwd" else ["grad_value"] + gproj + ["grad_ref"]
    names += list("BIHDQLP") + ["ref_dim", "pad", "align"] + (["mlc"] if direction == "bwd" else []) + ["stride"]
    names += ["ws", "wsb"] if direction == "bwd" else []
    return names + ["stream"]


def _elem(name, suffix):
    es, ves, ss = SIZES[suffix]
    if name in ("value", "grad_value"):
        return ves
    if name == "shapes":
        return 8
    return es if name in ("ref", "grad_ref") else ss


def _call(lib, direction, suffix, split=True, **over):
    buf = ctypes.create_string_buffer(4096 + 512)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    vals = dict(DIMS, ref_dim=2, pad=0, align=0, mlc=0, stride=0, ws=None, wsb=0, stream=None)
    vals.update({n: p for n in BUFFERS})
    vals.update({k: (p + v[1] if isinstance(v, tuple) else v) for k, v in over.items()})
    fn = getattr(lib, f"msda_{direction}_fused_levelref_{'split_' if split else ''}{suffix}")
    names = _spec(direction, split)
    assert len(names) == len(fn.argtypes)
    rc = fn(*[vals[n] for n in names])
    del buf
    return rc


def _rows(direction, suffix):
    """(label, overrides, status, message keyword or None, does the interleaved twin see the same row?)"""
    inputs = (["grad_out"] if direction == "bwd" else []) + ["value", "shapes", "offsets", "logits", "ref"]
    outputs = ["out"] if direction == "fwd" else ["grad_value", "grad_offsets", "grad_logits", "grad_ref"]
    twin_has = lambda n: n not in ("logits", "grad_logits")  # noqa: E731
    rows = []
    for n in "BIHDQLP":
        rows.append((f"{n}=-1", {n: -1}, BAD_ARG, None, True))
    for n in inputs + [o for o in outputs if o != "grad_value"]:
        rows.append((f"{n}=NULL", {n: None}, BAD_ARG, None, twin_has(n)))
    for rd in (0, 1, 3, 5, -2):
        rows.append((f"ref_dim={rd}", {"ref_dim": rd}, BAD_ARG, "ref_dim", True))
    rows.append(("padding_mode=7", {"pad": 7}, BAD_ARG, None, True))
    rows.append(("L=33", {"L": 33}, TOO_MANY_LEVELS, None, True))
    rows.append(("I too large", {"I": 1 << 24}, TOO_LARGE, None, True))
    rows.append(("Q too large", {"Q": 1 << 24}, TOO_LARGE, None, True))
    rows.append(("too large with a null input", {"I": 1 << 24, "value": None}, TOO_LARGE, None, True))
    # the interleaved pair's bound on the projection: Q * H * L * P * 3 < 2^31 (the split pair keeps every guard of its twin)
    rows.append(("projection past 32-bit sample offsets", {"Q": (1 << 24) - 1, "P": 64}, TOO_LARGE, None, True))
    for n in inputs + outputs:
        rows.append((f"{n}+half", {n: ("shift", _elem(n, suffix) // 2)}, MISALIGNED, "misaligned", twin_has(n)))
    # (L * P beyond msda_fused_lp_limit is answered behind a question to the device — the launch plan reads its CU count —
    # so MSDA_ERR_UNSUPPORTED is held on the GPU: tests/test_gpu_levelref_split.py)
    base = {"grad_value": None} if direction == "bwd" else {}
    if direction == "bwd":
        rows += [("ws=NULL", {"ws": None, "wsb": 1 << 20}, BAD_ARG, "workspace", True),
                 ("ws misaligned", {"ws": ("shift", 128), "wsb": 1 << 20}, BAD_ARG, "workspace", True)]
    dense = DIMS["H"] * DIMS["D"] * SIZES[suffix][1]
    rows += [("stride negative", dict(base, stride=-dense), BAD_ARG, None, True),
             ("stride below the dense row", dict(base, stride=dense - SIZES[suffix][1]), BAD_ARG, None, True)]
    nulls = {n: None for n in BUFFERS}
    rows.append(("B=0, buffers NULL", dict(nulls, B=0), 0, None, True))
    if direction == "fwd":
        rows.append(("Q=0, buffers NULL", dict(nulls, Q=0), 0, None, True))
    return rows


@no_gpu
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_argument_errors_are_the_twins_and_answered_before_anything_is_launched(lib, direction):
    for suffix in SUFFIXES:
        for label, over, want, word, twin_sees in _rows(direction, suffix):
            assert lib.msda_get_option(b"no such option") == -1  # (leaves its own text behind: the next one is this call's)
            stale = lib.msda_last_error()
            rc = _call(lib, direction, suffix, **over)
            msg = lib.msda_last_error()
            where = (label, direction, suffix, rc, msg)
            assert rc == want, where
            if want != 0:
                assert msg and msg != stale, where
                if word is not None:
                    assert re.search(word, msg.decode()), where
            if twin_sees:  # the same row on the interleaved pair: the same answer
                assert _call(lib, direction, suffix, split=False, **over) == want, where


# ------------------------------------------------------------------------------------------------ the host definition
LEVELS = [(6, 4), (3, 2), (2, 5)]


def _core_inputs(dtype, ref_dim, seed=0, B=2, Q=7, H=2, D=5, P=3):
    g = torch.Generator().manual_seed(seed)
    L, I = len(LEVELS), sum(h * w for h, w in LEVELS)  # noqa: E741
    img = torch.randn(B, I, H, D, generator=g, dtype=dtype)
    off = torch.randn(B, Q, H, L, P, 2, generator=g, dtype=dtype)
    lgt = torch.randn(B, Q, H, L, P, generator=g, dtype=dtype)
    ref = torch.rand(B, Q, L, ref_dim, generator=g, dtype=dtype)
    vm = torch.rand(B, I, generator=g) > 0.2
    qm = torch.rand(B, Q, generator=g) > 0.3
    return img, torch.tensor(LEVELS), off, lgt, ref, vm, qm


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_host_core_is_the_interleaved_core_on_the_stacked_projection(dtype, ref_dim, masked):
    img, shapes, off, lgt, ref, vm, qm = _core_inputs(dtype, ref_dim)
    kw = dict(value_mask=vm, query_mask=qm) if masked else {}
    leaves = [t.clone().requires_grad_(True) for t in (img, off, lgt, ref)]
    out = fused_hf_module_core_split(leaves[0], shapes, leaves[1], leaves[2], leaves[3], "zeros", False, **kw)
    twin = [t.clone().requires_grad_(True) for t in (img, off, lgt, ref)]
    want = fused_hf_module_core(twin[0], shapes, torch.cat([twin[1], twin[2][..., None]], -1), twin[3], "zeros", False, **kw)
    assert torch.equal(out, want)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=dtype)
    (out * w).sum().backward()
    (want * w).sum().backward()
    for a, b in zip(leaves, twin):
        assert torch.equal(a.grad, b.grad)
    # the layers' own layouts: flat offsets, [B, Q, H, L*P] and flat logits
    B, Q, H, L, P, _ = off.shape
    for o2, l2 in ((off.reshape(B, Q, -1), lgt.reshape(B, Q, H, L * P)), (off, lgt.reshape(B, Q, -1))):
        assert torch.equal(fused_hf_module_core_split(img, shapes, o2, l2, ref, "zeros", False, **kw), out)


def test_split_views_and_their_errors():
    img, shapes, off, lgt, ref, _, _ = _core_inputs(torch.float32, 2)
    B, Q, H, L, P, _ = off.shape
    o, l = split_projection_views(off.reshape(B, Q, -1), lgt.reshape(B, Q, -1), H, L)  # noqa: E741
    assert o.shape == off.shape and l.shape == lgt.shape and o.data_ptr() == off.data_ptr() and l.data_ptr() == lgt.data_ptr()
    assert torch.equal(stack_split_projection(o, l)[..., :2], off) and torch.equal(stack_split_projection(o, l)[..., 2], lgt)
    with pytest.raises(ValueError, match="sampling_offsets"):
        split_projection_views(off.reshape(B, Q, -1)[..., :-1], lgt, H, L)
    with pytest.raises(ValueError, match="sampling_offsets"):
        split_projection_views(off[..., :1], lgt, H, L)
    with pytest.raises(ValueError, match="attention_logits"):
        split_projection_views(off, lgt[..., :-1], H, L)
    with pytest.raises(ValueError, match="attention_logits"):
        split_projection_views(off, lgt[:, :-1], H, L)


# ------------------------------------------------------------------------------------------------ the HF adapter
class LoraLikeLinear(torch.nn.Linear):
    """``.weight`` is the base weight; the adapter path lives in ``forward`` (what peft's lora.Linear does; after
    tests/test_linear_row_split.py's).  Both factors are non-zero, so the adapter path changes the output."""

    def __init__(self, i, o):
        super().__init__(i, o)
        self.a = torch.nn.Parameter(torch.randn(i, 2) * 0.3)
        self.b = torch.nn.Parameter(torch.randn(2, o) * 0.3)

    def forward(self, x):
        return super().forward(x) + (x @ self.a) @ self.b


def lora_wrap(layer: torch.nn.Linear) -> LoraLikeLinear:
    torch.manual_seed(17)
    new = LoraLikeLinear(layer.in_features, layer.out_features).to(layer.weight.device, layer.weight.dtype)
    with torch.no_grad():
        new.weight.copy_(layer.weight)
        new.bias.copy_(layer.bias)
    return new


DETR_LEVELS = [(6, 8), (3, 4), (2, 2), (1, 1)]


def detr_attention(seed=0):
    """A Deformable-DETR attention module from the local transformers, random weights everywhere (transformers
    zero-initialises the offsets' weight: the sampling pattern would not depend on the data)."""
    from transformers import DeformableDetrConfig, ResNetConfig
    from transformers.models.deformable_detr.modeling_deformable_detr import DeformableDetrMultiscaleDeformableAttention
    bb = ResNetConfig(num_channels=3, embedding_size=16, hidden_sizes=[16, 32, 64, 128], depths=[1, 1, 1, 1],
                      layer_type="basic", out_features=["stage2", "stage3", "stage4"])  # (never built: no download)
    cfg = DeformableDetrConfig(d_model=64, num_feature_levels=4, use_timm_backbone=False, use_pretrained_backbone=False,
                               backbone_config=bb, backbone=None)
    torch.manual_seed(seed)
    m = DeformableDetrMultiscaleDeformableAttention(cfg, num_heads=4, n_points=4)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape) * (0.1 if p.dim() == 2 else 0.5))
    return m


def detr_call(device="cpu", dtype=torch.float32, ref_dim=2):
    g = torch.Generator().manual_seed(1)
    n = sum(h * w for h, w in DETR_LEVELS)
    hidden, pos = torch.randn(2, n, 64, generator=g), torch.randn(2, n, 64, generator=g)
    ref = torch.rand(2, n, 4, ref_dim, generator=g)
    mask = torch.ones(2, n, dtype=torch.bool)
    mask[1, -5:] = False
    hidden = hidden.to(device, dtype)
    return hidden, dict(attention_mask=mask.to(device), encoder_hidden_states=hidden, position_embeddings=pos.to(device, dtype),
                        reference_points=ref.to(device, dtype), spatial_shapes=torch.tensor(DETR_LEVELS, device=device),
                        spatial_shapes_list=DETR_LEVELS, level_start_index=None)


def run_attention(m, hidden, kw):
    """(output, {parameter name: gradient}) of one call under a fixed random linear functional of the output"""
    m.zero_grad(set_to_none=True)
    hidden = hidden.detach().requires_grad_(True)
    kw = dict(kw)
    if kw.get("encoder_hidden_states") is not None:
        kw["encoder_hidden_states"] = hidden
    out = m(hidden, **kw)[0]
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(11)).to(out.device)
    (out.float() * w).sum().backward()
    grads = {k: p.grad.detach().float().clone() for k, p in m.named_parameters()}
    grads["hidden_states"] = hidden.grad.detach().float().clone()
    return out.detach().float(), grads


def assert_same_call(got, want, atol=1e-5, rtol=1e-4, gtol=1e-4):
    torch.testing.assert_close(got[0], want[0], atol=atol, rtol=rtol)
    assert set(got[1]) == set(want[1])
    for k, g in want[1].items():
        err = float((got[1][k] - g).norm() / g.norm().clamp_min(1e-30))
        assert err < gtol, (k, err)


def make_not_plain(m, how):
    """``lora``: the offsets layer becomes a LoRA-like subclass; ``hook``: a forward hook scales the logits.  Returns what
    the original forward of the SAME module gives afterwards (the reference) is computed by the caller."""
    if how == "lora":
        m.sampling_offsets = lora_wrap(m.sampling_offsets)
        assert not _linear._plain_linear(m.sampling_offsets)
    else:
        m.attention_weights.register_forward_hook(lambda mod, args, out: out * 1.5)
        assert not _linear._plain_linear(m.attention_weights)


@pytest.mark.parametrize("how", ["lora", "hook"])
def test_fused_adapter_calls_layers_that_are_not_plain(how):
    """Fails on the parent commit: its fused forward reads ``.weight`` / ``.bias`` and returns the base weights' result."""
    pytest.importorskip("transformers")
    from msda_triton_amd.hf_adapter import FusedHFDeformableAttention, replace_hf_msda
    holder = torch.nn.ModuleDict({"attn": detr_attention()})
    make_not_plain(holder["attn"], how)
    hidden, kw = detr_call()
    base = detr_attention()  # the same weights without the adapter path / the hook: the result must NOT be this one
    want, plain = run_attention(holder["attn"], hidden, kw), run_attention(base, hidden, kw)
    assert float((want[0] - plain[0]).abs().max()) > 1e-2  # (the adapter path / the hook matters at these weights)
    keys = list(holder.state_dict().keys())
    assert replace_hf_msda(holder, fused=True) == 2  # the core swapped, the attention module wrapped
    assert isinstance(holder["attn"], FusedHFDeformableAttention) and list(holder.state_dict().keys()) == keys
    got = run_attention(holder["attn"], hidden, kw)
    if how == "lora":
        assert {"sampling_offsets.a", "sampling_offsets.b"} <= set(got[1])
    assert_same_call(got, want)


def test_plain_layers_keep_the_one_gemm_and_its_bias_error(monkeypatch):
    pytest.importorskip("transformers")
    from msda_triton_amd import hf_adapter
    holder = torch.nn.ModuleDict({"attn": detr_attention()})
    hidden, kw = detr_call()
    want = run_attention(holder["attn"], hidden, kw)
    hf_adapter.replace_hf_msda(holder, fused=True)
    called = []
    monkeypatch.setattr(hf_adapter, "fused_hf_module_core_split", lambda *a, **k: called.append(1))
    assert_same_call(run_attention(holder["attn"], hidden, kw), want)
    assert not called
    holder["attn"].attention_weights.bias = None
    with pytest.raises(ValueError, match="both have a bias or neither"):
        holder["attn"](hidden, **kw)


# ------------------------------------------------------------------------------------------------ Mask2Former, OneFormer
PIX_LEVELS = [(6, 8), (3, 4), (2, 3)]


def pixel_decoder_layer(kind, seed=0):
    """A tiny randomly initialised pixel-decoder encoder layer: (layer, name of its shapes argument)"""
    if kind == "mask2former":
        from transformers import Mask2FormerConfig
        from transformers.models.mask2former.modeling_mask2former import Mask2FormerPixelDecoderEncoderLayer as Layer
        cfg = Mask2FormerConfig(feature_size=32, num_attention_heads=4, encoder_feedforward_dim=64, dropout=0.0)
    else:
        from transformers import OneFormerConfig
        from transformers.models.oneformer.modeling_oneformer import OneFormerPixelDecoderEncoderLayer as Layer
        cfg = OneFormerConfig(conv_dim=32, num_attention_heads=4, encoder_feedforward_dim=64, dropout=0.0)
    torch.manual_seed(seed)
    layer = Layer(cfg)
    with torch.no_grad():
        for p in layer.self_attn.parameters():
            p.copy_(torch.randn(p.shape) * (0.15 if p.dim() == 2 else 0.5))
    import inspect
    names = inspect.signature(type(layer).forward).parameters
    return layer, ("spatial_shapes_list" if "spatial_shapes_list" in names else "spatial_shapes")


def pixel_decoder_call(shapes_arg, device="cpu", dtype=torch.float32):
    g = torch.Generator().manual_seed(2)
    n = sum(h * w for h, w in PIX_LEVELS)
    hidden, pos = torch.randn(2, n, 32, generator=g), torch.randn(2, n, 32, generator=g)
    ref = torch.rand(2, n, 3, 2, generator=g)
    # True = PADDING (the inverse of Deformable-DETR's polarity): the last columns of every level of the second image
    pad = torch.zeros(2, n, dtype=torch.bool)
    start = 0
    for h, w in PIX_LEVELS:
        cols = torch.arange(h * w) % w
        pad[1, start:start + h * w] = cols >= w - max(1, w // 4)
        start += h * w
    shapes = PIX_LEVELS if shapes_arg == "spatial_shapes_list" else torch.tensor(PIX_LEVELS, device=device)
    kw = {"attention_mask": pad.to(device), "position_embeddings": pos.to(device, dtype),
          "reference_points": ref.to(device, dtype), shapes_arg: shapes, "level_start_index": None}
    return hidden.to(device, dtype), kw, pad


@pytest.mark.parametrize("fused", [False, True], ids=["core", "fused"])
@pytest.mark.parametrize("kind", ["mask2former", "oneformer"])
def test_pixel_decoder_layers_are_reached(kind, fused):
    """Fails on the parent commit: ``replace_hf_msda`` returns 0 for these models."""
    pytest.importorskip("transformers")
    from msda_triton_amd import hf_adapter
    layer, shapes_arg = pixel_decoder_layer(kind)
    hidden, kw, pad = pixel_decoder_call(shapes_arg)
    assert pad[1].any() and not pad[0].any()
    want = run_attention(layer, hidden, kw)
    nomask = run_attention(layer, hidden, dict(kw, attention_mask=None))
    assert float((want[0] - nomask[0]).abs().max()) > 1e-3  # (the padded columns matter)
    keys = list(layer.state_dict().keys())
    assert hf_adapter.replace_hf_msda(layer, fused=fused) == 1
    assert list(layer.state_dict().keys()) == keys
    assert isinstance(layer.self_attn, hf_adapter.HFPixelDecoderDeformableAttention)
    assert isinstance(layer.self_attn, hf_adapter.FusedHFDeformableAttention) == fused
    assert hf_adapter.replace_hf_msda(layer, fused=fused) == 0  # idempotent
    assert_same_call(run_attention(layer, hidden, kw), want)
    assert_same_call(run_attention(layer, hidden, dict(kw, attention_mask=None)), nomask)
    # attention weights on request: the original forward
    attn_kw = {k: v for k, v in kw.items()}
    out, w = layer.self_attn(hidden, encoder_hidden_states=hidden, output_attentions=True, **attn_kw)
    assert w is not None and w.shape[-2:] == (3, 4)
    out2, w2 = layer.self_attn(hidden, encoder_hidden_states=hidden, **attn_kw)
    torch.testing.assert_close(out2, out, atol=1e-5, rtol=1e-4)
    assert (w2 is None) == fused


@pytest.mark.parametrize("how", ["lora", "hook"])
def test_fused_pixel_decoder_layer_behind_layers_that_are_not_plain(how):
    pytest.importorskip("transformers")
    from msda_triton_amd import hf_adapter
    layer, shapes_arg = pixel_decoder_layer("mask2former")
    make_not_plain(layer.self_attn, how)
    hidden, kw, _ = pixel_decoder_call(shapes_arg)
    want = run_attention(layer, hidden, kw)
    assert hf_adapter.replace_hf_msda(layer, fused=True) == 1
    assert_same_call(run_attention(layer, hidden, kw), want)


def test_upgrade_from_the_core_to_the_fused_wrapper():
    pytest.importorskip("transformers")
    from msda_triton_amd import hf_adapter
    layer, _ = pixel_decoder_layer("mask2former")
    assert hf_adapter.replace_hf_msda(layer) == 1 and hf_adapter.replace_hf_msda(layer, fused=True) == 1
    assert isinstance(layer.self_attn, hf_adapter.FusedHFPixelDecoderDeformableAttention)
    assert hf_adapter.replace_hf_msda(layer) == 0 and hf_adapter.replace_hf_msda(layer, fused=True) == 0
