"""GPU: every autograd node of the C++ binding (csrc/msda_torch_ext.cpp), called as `ext.<name>(...)` with the arguments
the Python callers pass, against the Python autograd Function of the same family called with `.apply` — both are glue
over the same C ABI, so they launch the same kernels on the same buffers.  The tests hold the glue, not the kernels (those
are held elsewhere): which entry point a dtype pair reaches, what is saved for the backward, which gradients are
allocated and returned, the value-row stride, the cast of grad_out, once_differentiable.  One small pyramid with three
levels, unequal per-level counts, several heads and B > 1 is the smallest shape at which any of that can go wrong.

Bounds, each taken from the family's existing route test:
  * msda: outputs and sample gradients `torch.equal`, grad_value `atol = rtol = 1e-5`
    (test_gpu_parity.py::test_cpp_binding_and_ctypes_routes_agree);
  * msda_ragged: `torch.equal` (test_ragged_points.py::test_gpu_cpp_route_and_python_route_agree);
  * msda_discrete: `torch.equal`
    (test_discrete_sampling.py::test_gpu_cpp_node_function_and_torch_compile_route_agree_bitwise);
  * msda_fused_ragged: `torch.equal` (test_gpu_fused_ragged.py::test_cpp_node_and_python_function_agree_bit_for_bit);
  * msda_fused_levelref, and msda_fused, whose Python Function goes through the same launcher (msda_hip_fwd_fused /
    msda_hip_bwd_fused): `torch.equal`
    (test_gpu_hf_fused.py::test_cpp_node_python_function_and_ctypes_launch_agree_bit_for_bit);
  * msda_fused_hfbox: `torch.equal`
    (test_gpu_hf_box_fused.py::test_cpp_node_python_function_and_ctypes_launch_agree_bit_for_bit)."""
import functools

import pytest
import torch

from msda_triton_amd import _ext, _lib, discrete, functional, ragged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LEVELS = [(6, 5), (3, 4), (2, 2)]
B, Q, H, D, P = 2, 21, 4, 8, 4
COUNTS = (3, 6, 3)
# nine samples per unit: the most the fused kernels' backward takes in fp64 at this head dimension (see the dtype test)
P_SMALL, COUNTS_SMALL = 3, (2, 4, 3)
I = sum(h * w for h, w in LEVELS)  # noqa: E741
L = len(LEVELS)
OFFSET_SCALE = 0.3
F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
# (value dtype, dtype of every other tensor): the six pairs the binding's dtype table serves
DTYPES = {"f32": (F32, F32), "f64": (F64, F64), "f16": (F16, F16), "bf16": (BF16, BF16), "vbf16_f32": (BF16, F32),
          "vf16_f32": (F16, F32)}


@pytest.fixture(scope="module")
def ext():
    mod = _ext.load()
    if mod is None:
        pytest.skip("msda_torch_ext is not built (optional)")
    return mod


def _pad(pm):
    return _lib.PADDING_MODES[pm]


# name of the binding's function -> (node class, fused?, per-level counts?, reference-point shapes by ref_dim,
#                                    call of the binding, call of the Python Function)
NODES = {
    "msda": dict(
        cls="MSDAFunction", fused=False, counts=False,
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda(v, s, a, b, _pad(pm), bool(ac), 0),
        py=lambda v, s, a, b, pm, ac, n: functional._HipMultiscaleDeformableAttentionFunction.apply(v, s, a, b, pm, ac, 0)),
    "msda_ragged": dict(
        cls="MSDARaggedFunction", fused=False, counts=True,
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_ragged(v, s, a, b, _pad(pm), bool(ac), 0, list(n)),
        py=lambda v, s, a, b, pm, ac, n: ragged._HipRaggedFunction.apply(v, s, a, b, pm, ac, n, 0)),
    "msda_discrete": dict(
        cls="MSDADiscreteFunction", fused=False, counts=True,
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_discrete(v, s, a, b, 0, list(n)),
        py=lambda v, s, a, b, pm, ac, n: discrete._HipDiscreteFunction.apply(v, s, a, b, n, 0)),
    "msda_fused": dict(
        cls="MSDAFusedFunction", fused=True, counts=False, ref=lambda r: (B, Q, r),
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_fused(v, s, a, b, _pad(pm), bool(ac), 0),
        py=lambda v, s, a, b, pm, ac, n: functional._HipFusedModuleCoreFunction.apply(v, s, a, b, pm, ac, 0)),
    "msda_fused_ragged": dict(
        cls="MSDAFusedRaggedFunction", fused=True, counts=True, ref=lambda r: (B, Q, r),
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_fused_ragged(v, s, a, b, _pad(pm), bool(ac), 0, list(n)),
        py=lambda v, s, a, b, pm, ac, n: ragged._HipFusedRaggedModuleCoreFunction.apply(v, s, a, b, pm, ac, n, 0)),
    "msda_fused_hfbox": dict(
        cls="MSDAFusedHfBoxFunction", fused=True, counts=True, ref=lambda r: (B, Q, 4),
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_fused_hfbox(v, s, a, b, _pad(pm), bool(ac), 0, list(n),
                                                             list(functional.hf_box_level_scale(n)), OFFSET_SCALE),
        py=lambda v, s, a, b, pm, ac, n: ragged._HipFusedHfBoxCoreFunction.apply(v, s, a, b, pm, ac, n, OFFSET_SCALE, 0)),
    "msda_fused_levelref": dict(
        cls="MSDAFusedLevelRefFunction", fused=True, counts=False, ref=lambda r: (B, Q, L, r),
        ext=lambda e, v, s, a, b, pm, ac, n: e.msda_fused_levelref(v, s, a, b, _pad(pm), bool(ac), 0),
        py=lambda v, s, a, b, pm, ac, n: functional._HipFusedHFModuleCoreFunction.apply(v, s, a, b, pm, ac, 0)),
}


def _cases():
    out = []
    for name, node in NODES.items():
        ref_dims = (4,) if name == "msda_fused_hfbox" else (2, 4) if node["fused"] else (0,)
        modes = (("zeros", False),) if name == "msda_discrete" else (("zeros", False), ("border", True))  # (no padding mode)
        out += [pytest.param(name, r, pm, ac, id=f"{name}-ref{r}-{pm}_{int(ac)}" if r else f"{name}-{pm}_{int(ac)}")
                for r in ref_dims for pm, ac in modes]
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def make(name, ref_dim, dtype_key, small=False):
    """(value, shapes, third, fourth, grad_out) on the GPU; shared between the tests, which never write to them"""
    node = NODES[name]
    vdt, cdt = DTYPES[dtype_key]
    g = torch.Generator(device="cpu").manual_seed(sum(name.encode()) + 7 * ref_dim)
    samples = (sum(COUNTS_SMALL if small else COUNTS),) if node["counts"] else (L, P_SMALL if small else P)
    value = torch.randn(B, I, H, D, generator=g, dtype=F64).to(vdt)
    if node["fused"]:
        third = (torch.randn(B, Q, H, *samples, 3, generator=g, dtype=F64) * 1.5).to(cdt)
        fourth = torch.rand(*node["ref"](ref_dim), generator=g, dtype=F64).to(cdt)
    else:
        third = (torch.rand(B, Q, H, *samples, 2, generator=g, dtype=F64) * 1.2 - 0.1).to(cdt)  # some samples outside
        fourth = torch.rand(B, Q, H, *samples, generator=g, dtype=F64).to(cdt)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=F64).to(cdt)
    return tuple(t.to(DEV) for t in (value, torch.tensor(LEVELS), third, fourth, gout))


def run(call, value, shapes, third, fourth, gout, needs=(True, True, True)):
    """out and the three `.grad`s (None where autograd left none)"""
    v, a, b = (t.detach().requires_grad_(n) for t, n in zip((value, third, fourth), needs))  # (detach: keeps the strides)
    out = call(v, shapes, a, b)
    out.backward(gout)
    return out.detach(), v.grad, a.grad, b.grad


def assert_same(name, got, want):
    for what, x, y in zip(("out", "grad_value", "grad_third", "grad_fourth"), got, want):
        assert (x is None) == (y is None), (name, what, "the node" if x is None else "the Python Function", "left no gradient")
        if x is None:
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, (name, what, x.dtype, y.dtype, x.shape, y.shape)
        if name == "msda" and what == "grad_value":
            torch.testing.assert_close(x, y, atol=1e-5, rtol=1e-5, msg=lambda m: f"{name} {what}: {m}")
        else:
            assert torch.equal(x, y), (name, what, float((x.double() - y.double()).abs().max()))


def calls(ext, name, pm, ac, counts=COUNTS):
    node = NODES[name]
    return (lambda v, s, a, b: node["ext"](ext, v, s, a, b, pm, ac, counts)), \
        (lambda v, s, a, b: node["py"](v, s, a, b, pm, ac, counts))


@pytest.mark.parametrize("dtype_key", list(DTYPES))
@pytest.mark.parametrize("name,ref_dim,pm,ac", CASES)
def test_every_dtype_pair_reaches_the_python_functions_entry_point(ext, name, ref_dim, pm, ac, dtype_key):
    """The fused nodes in fp64 at this shape: 12 samples per unit are within the fused forward's LDS pass and beyond the
    fused backward's (msda_fused_lp_limit(8, 8) = 9: 'fused prologue needs all L*P=12 samples of a unit in LDS at once
    (limit 9)').  The Python callers check that limit and never hand such a call to the node, which does not compose: its
    forward is the Python Function's and its backward raises the library's refusal under the family's name.  The
    gradients of the fp64 entry points are held at nine samples per unit (P = 3, counts [2, 4, 3])."""
    node_call, py_call = calls(ext, name, pm, ac)
    c = make(name, ref_dim, dtype_key)
    vdt, cdt = DTYPES[dtype_key]
    if NODES[name]["fused"] and L * P > int(ext.fused_lp_limit(D, c[2].element_size())):
        assert dtype_key == "f64"
        v, a, b = (t.detach().requires_grad_(True) for t in (c[0], c[2], c[3]))
        out = node_call(v, c[1], a, b)
        assert torch.equal(out, py_call(c[0], c[1], c[2], c[3]))
        with pytest.raises(ValueError, match=rf"msda_bwd{name[4:]}: rejected arguments \(-5\)"):
            out.backward(c[4])
        node_call, py_call = calls(ext, name, pm, ac, COUNTS_SMALL)
        c = make(name, ref_dim, dtype_key, small=True)
        assert L * P_SMALL == sum(COUNTS_SMALL) <= int(ext.fused_lp_limit(D, c[2].element_size()))
    got, want = run(node_call, *c), run(py_call, *c)
    assert got[0].dtype == cdt and got[1].dtype == vdt
    assert_same(name, got, want)


def need_patterns(name):
    if name == "msda_discrete":  # (no gradient for the sampling points in this mode)
        return {"all": (True, True, True), "value_only": (True, False, False), "weights_only": (False, False, True)}
    return {"all": (True, True, True), "value_frozen": (False, True, True), "third_only": (False, True, False),
            "fourth_only": (False, False, True)}


@pytest.mark.parametrize("name,ref_dim,pm,ac", CASES)
def test_partial_needs_leave_the_python_functions_pattern_of_gradients(ext, name, ref_dim, pm, ac):
    node_call, py_call = calls(ext, name, pm, ac)
    c = make(name, ref_dim, "f32")
    for pattern, needs in need_patterns(name).items():
        got, want = run(node_call, *c, needs=needs), run(py_call, *c, needs=needs)
        for x, n in zip(got[1:], needs):
            assert x is None or n, (name, pattern)
        if name == "msda_discrete":
            assert got[2] is None
        assert_same(f"{name}", got, want)
    out = node_call(*c[:4])  # nothing requires a gradient
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out, want[0])


@pytest.mark.parametrize("name,ref_dim,pm,ac", CASES)
def test_value_rows_and_grad_out_layouts_give_the_dense_result(ext, name, ref_dim, pm, ac):
    node_call, _ = calls(ext, name, pm, ac)
    value, shapes, third, fourth, gout = make(name, ref_dim, "f32")
    want = run(node_call, value, shapes, third, fourth, gout)

    def same(got, what):
        for x, y in zip(got, want):
            assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), (name, what)

    # a padded pyramid is read in place, forward and backward (the stride saved for the backward); grad_value is dense
    padded = functional.padded_value_rows(B, I, H, D, F32, DEV, pad_bytes=16)
    padded.copy_(value)
    assert not padded.is_contiguous()
    got = run(node_call, padded, shapes, third, fourth, gout)
    assert got[1].is_contiguous()
    same(got, "padded value rows")
    # grad_out as a non-contiguous view
    wide = torch.empty(B, Q, H, 2 * D, device=DEV)
    wide[..., ::2] = gout
    assert not wide[..., ::2].is_contiguous()
    same(run(node_call, value, shapes, third, fourth, wide[..., ::2]), "strided grad_out")
    # grad_out in fp64 next to an fp32 op (the fp32 values widened: the cast back is exact)
    same(run(node_call, value, shapes, third, fourth, gout.double()), "fp64 grad_out")


@pytest.mark.parametrize("name", list(NODES))
def test_node_class_names_and_double_backward_raises(ext, name):
    ref_dim = 4 if NODES[name]["fused"] else 0
    node_call, _ = calls(ext, name, "zeros", False)
    value, shapes, third, fourth, gout = make(name, ref_dim, "f32")
    v, a, b = (t.detach().requires_grad_(True) for t in (value, third, fourth))
    out = node_call(v, shapes, a, b)
    assert NODES[name]["cls"] in out.grad_fn.name()
    g = gout.clone().requires_grad_()
    out.backward(g, create_graph=True)
    grad = b.grad  # (the weights / the reference points: every node has this gradient)
    v.grad = a.grad = b.grad = None
    assert grad is not None and grad.requires_grad
    with pytest.raises(RuntimeError, match="differentiate twice"):
        grad.sum().backward()
