"""The query padding mask (``query_mask=``) without a GPU: the composed route — which is the definition of the feature on
host tensors — against the CPU oracle on sanitised inputs, its gradients, containment of non-finite values in masked
queries, the argument checks, the new C-ABI symbols, and the promises of the mask generators the GPU file uses.

The contract (include/msda_hip.h, "QUERY PADDING MASK"; ``plain`` = the same call without ``query_mask``):

    real queries     rows of out, grad_loc, grad_attn (grad_proj, grad_ref) equal plain's, bit for bit
    masked queries   those rows are zeros
    grad_value       the sum over the real queries' samples; no bit of a masked query's inputs reaches any output

``sanitised`` inputs: masked queries hold points 0.5, weights (or logits and offsets) 0 and a zero grad_out row."""
import ctypes

import numpy as np
import pytest
import torch

import query_mask_cases as qmc
from conftest import MODES, kink_mask, mode_key
from msda_triton_amd import MultiscaleDeformableAttention, _lib, functional
from msda_triton_amd.functional import (apply_query_mask, fused_hf_box_core, fused_hf_module_core, fused_module_core,
                                        multiscale_deformable_attention)
from test_value_mask import I, LEVELS, TOL, _case, _grads, _hf_inputs, _mask

F64 = TOL[torch.float64]


def _qmask(B, Q, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    m = torch.rand(B, Q, generator=g) < 0.55
    m[0, 0] = False  # (the first query is always among the masked, the last among the real ones)
    m[-1, -1] = True
    return m


def _rows(t, m):
    return m.reshape(m.shape + (1,) * (t.dim() - 2))


def _sanitise(loc, attn, go, m):
    return (torch.where(_rows(loc, m), loc, torch.full_like(loc, 0.5)), torch.where(_rows(attn, m), attn, torch.zeros_like(attn)),
            torch.where(_rows(go, m), go, torch.zeros_like(go)))


def _assert_rows(got, plain, m, names):
    """real queries' rows equal plain's bit for bit, masked queries' rows are zeros"""
    for nm, g, w in zip(names, got, plain):
        if g is None and w is None:
            continue
        sel = _rows(g, m).expand_as(g)
        assert torch.equal(g[sel], w[sel]), nm
        assert (g[~sel] == 0).all(), nm


# ------------------------------------------------------------------------------------------ the composed route, fp64
@pytest.mark.parametrize("pm,ac", MODES, ids=[mode_key(*m) for m in MODES])
def test_host_operator_against_the_oracle_on_sanitised_inputs(oracle, pm, ac):
    value, shapes, loc, attn, go = _case(torch.float64)
    m = _qmask(value.shape[0], loc.shape[1])
    for vm in (None, _mask(value.shape[0])):
        def op(v, l, a, **kw):
            return multiscale_deformable_attention(v, shapes, l, a, pm, ac, value_mask=vm, **kw)

        for mask in (m, m.to(torch.uint8)):
            got = _grads(lambda v, l, a: op(v, l, a, query_mask=mask), (value, loc, attn), go)
        plain = _grads(op, (value, loc, attn), go)
        _assert_rows((got[0], got[2], got[3]), (plain[0], plain[2], plain[3]), m, ("out", "grad_loc", "grad_attn"))
        # the oracle on the sanitised inputs (and the pre-masked value)
        s_loc, s_attn, s_go = _sanitise(loc, attn, go, m)
        v_ref = value if vm is None else torch.where(vm[:, :, None, None], value, torch.zeros_like(value))
        host = [t.numpy() for t in (v_ref, shapes, s_loc, s_attn)]
        (fa, fr), (ba, br) = F64["fwd"], F64["bwd"]
        np.testing.assert_allclose(got[0].numpy(), oracle.forward(*host, pm, ac), atol=fa, rtol=fr)
        r_gv, r_gl, r_ga = oracle.backward(s_go.numpy(), *host, pm, ac)
        if vm is not None:
            r_gv = np.where(vm[:, :, None, None].numpy(), r_gv, 0)
        np.testing.assert_allclose(got[1].numpy(), r_gv, atol=ba, rtol=br)
        real = m[:, :, None, None, None].numpy()
        np.testing.assert_allclose(got[3].numpy(), np.where(real, r_ga, 0), atol=ba, rtol=br)
        keep = ~kink_mask(s_loc.numpy(), shapes.numpy(), ac) & real[..., None]
        np.testing.assert_allclose(np.where(keep, got[2].numpy(), 0), np.where(keep, r_gl, 0), atol=ba, rtol=br)
        # grad_value is plain's on the sanitised inputs, bit for bit: the composition IS that call
        want = _grads(op, (value, s_loc, s_attn), s_go)
        assert torch.equal(got[1], want[1])


@pytest.mark.parametrize("pm,ac", MODES, ids=[mode_key(*m) for m in MODES])
def test_points_per_level_route_against_the_oracle(oracle, pm, ac):
    """per-level counts (3, 1, 2): the oracle takes them as the uniform call with P = 3 and weight 0 in the padding samples"""
    counts = (3, 1, 2)
    value, shapes, _, _, go = _case(torch.float64, seed=1)
    g = torch.Generator().manual_seed(5)
    B, Q, H = value.shape[0], go.shape[1], value.shape[2]
    loc = torch.rand(B, Q, H, sum(counts), 2, generator=g, dtype=torch.float64) * 1.4 - 0.2
    attn = torch.rand(B, Q, H, sum(counts), generator=g, dtype=torch.float64)
    m = _qmask(B, Q, 1)

    def op(v, l, a, **kw):
        return multiscale_deformable_attention(v, shapes, l, a, pm, ac, points_per_level=counts, **kw)

    got = _grads(lambda v, l, a: op(v, l, a, query_mask=m), (value, loc, attn), go)
    plain = _grads(op, (value, loc, attn), go)
    _assert_rows((got[0], got[2], got[3]), (plain[0], plain[2], plain[3]), m, ("out", "grad_loc", "grad_attn"))
    s_loc, s_attn, s_go = _sanitise(loc, attn, go, m)
    P = max(counts)
    d_loc = torch.full((B, Q, H, len(counts), P, 2), 0.5, dtype=torch.float64)
    d_attn = torch.zeros(B, Q, H, len(counts), P, dtype=torch.float64)
    start = 0
    for l, n in enumerate(counts):
        d_loc[:, :, :, l, :n] = s_loc[:, :, :, start:start + n]
        d_attn[:, :, :, l, :n] = s_attn[:, :, :, start:start + n]
        start += n
    host = [t.numpy() for t in (value, shapes, d_loc, d_attn)]
    (fa, fr), (ba, br) = F64["fwd"], F64["bwd"]
    np.testing.assert_allclose(got[0].numpy(), oracle.forward(*host, pm, ac), atol=fa, rtol=fr)
    r_gv, _, r_ga = oracle.backward(s_go.numpy(), *host, pm, ac)
    np.testing.assert_allclose(got[1].numpy(), r_gv, atol=ba, rtol=br)
    start = 0
    for l, n in enumerate(counts):
        np.testing.assert_allclose(got[3][:, :, :, start:start + n].numpy(),
                                   np.where(m[:, :, None, None].numpy(), r_ga[:, :, :, l, :n], 0), atol=ba, rtol=br)
        start += n


def test_discrete_route_composes():
    """nearest-pixel sampling has no oracle entry of its own: the composed route against the discrete operator on the
    sanitised inputs (held to its own reference by tests/test_discrete_sampling.py), in fp64"""
    value, shapes, loc, attn, go = _case(torch.float64, seed=2)
    m = _qmask(value.shape[0], loc.shape[1], 2)

    def run(v, a, l=loc, **kw):
        return multiscale_deformable_attention(v, shapes, l, a, "border", False, sampling_mode="discrete", **kw)

    got = _grads(lambda v, a: run(v, a, query_mask=m), (value, attn), go)
    plain = _grads(run, (value, attn), go)
    _assert_rows((got[0], got[2]), (plain[0], plain[2]), m, ("out", "grad_attn"))
    s_loc, s_attn, s_go = _sanitise(loc, attn, go, m)
    want = _grads(lambda v, a: run(v, a, l=s_loc), (value, s_attn), s_go)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])


@pytest.mark.parametrize("ref_dim", [2, 4])
def test_fused_cores_and_the_module_compose(ref_dim):
    value, shapes, proj, ref, go = _hf_inputs(ref_dim, dtype=torch.float64)
    B, Q = proj.shape[:2]
    m = _qmask(B, Q, 3)
    vm = _mask(B, 3)
    names = ("out", "grad_proj", "grad_ref")
    for kw in ({}, {"mask_in_kernels": False}, {"value_mask": vm}):
        def hf(v, p, r, **k2):
            return fused_hf_module_core(v, shapes, p, r, "zeros", False, **kw, **k2)

        got = _grads(lambda v, p, r: hf(v, p, r, query_mask=m), (value, proj, ref), go)
        plain = _grads(hf, (value, proj, ref), go)
        _assert_rows((got[0], got[2], got[3]), (plain[0], plain[2], plain[3]), m, names)
        s_proj, s_ref, s_go = qmc.sanitised_fused(proj, ref, go, m)
        assert torch.equal(got[1], _grads(hf, (value, s_proj, s_ref), s_go)[1])
    ref1 = ref[:, :, 0].contiguous()
    got = _grads(lambda v, p, r: fused_module_core(v, shapes, p, r, "border", True, query_mask=m), (value, proj, ref1), go)
    plain = _grads(lambda v, p, r: fused_module_core(v, shapes, p, r, "border", True), (value, proj, ref1), go)
    _assert_rows((got[0], got[2], got[3]), (plain[0], plain[2], plain[3]), m, names)
    if ref_dim == 4:
        counts = (3, 1, 2)
        g = torch.Generator().manual_seed(6)
        bproj = torch.randn(B, Q, value.shape[2], sum(counts), 3, generator=g, dtype=torch.float64)
        box = torch.rand(B, Q, 4, generator=g, dtype=torch.float64)
        got = _grads(lambda v, p, r: fused_hf_box_core(v, shapes, p, r, counts, query_mask=m), (value, bproj, box), go)
        plain = _grads(lambda v, p, r: fused_hf_box_core(v, shapes, p, r, counts), (value, bproj, box), go)
        _assert_rows((got[0], got[2], got[3]), (plain[0], plain[2], plain[3]), m, names)


def test_nn_module_gives_masked_queries_the_output_bias():
    torch.manual_seed(0)
    mod = MultiscaleDeformableAttention(16, 12, len(LEVELS), 3, 2, "zeros", False)
    g = torch.Generator().manual_seed(7)
    img, queries, ref = torch.randn(2, I, 16, generator=g), torch.randn(2, 5, 16, generator=g), torch.rand(2, 5, 2, generator=g)
    shapes = torch.tensor(LEVELS)
    m = _qmask(2, 5, 6)
    out = mod(img, shapes, queries, ref, query_mask=m)
    plain = mod(img, shapes, queries, ref)
    assert torch.equal(out[m], plain[m])
    assert torch.equal(out[~m], mod.query_output_proj.bias.expand_as(out[~m]))
    poisoned = torch.where(m[:, :, None], queries, torch.full_like(queries, float("nan")))
    assert torch.equal(mod(img, shapes, poisoned, ref, query_mask=m), out)


# ------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("levels", [[(3, 4)], [(2, 2)], [(3, 4), (2, 2)]], ids=["3x4", "2x2", "both"])
def test_gradcheck_fp64(levels):
    """B 2, Q 5, H 2, D 4, P 2; the points stay inside a cell (no kink of the bilinear weights within eps)"""
    B, Q, H, D, P, L = 2, 5, 2, 4, 2, len(levels)
    n = sum(h * w for h, w in levels)
    g = torch.Generator().manual_seed(11)
    value = torch.randn(B, n, H, D, generator=g, dtype=torch.float64)
    shapes = torch.tensor(levels)
    size = torch.tensor([[w, h] for h, w in levels], dtype=torch.float64)[:, None, :]      # [L, 1, (w, h)]
    cell = torch.floor(torch.rand(B, Q, H, L, P, 2, generator=g, dtype=torch.float64) * size)
    loc = (cell + 0.5 + 0.25 + 0.5 * torch.rand(B, Q, H, L, P, 2, generator=g, dtype=torch.float64)) / size  # pixel coord k + [.25, .75]
    attn = torch.rand(B, Q, H, L, P, generator=g, dtype=torch.float64)
    m = torch.tensor([[1, 0, 1, 1, 0], [0, 1, 1, 0, 1]], dtype=torch.bool)
    value.requires_grad_(True), loc.requires_grad_(True), attn.requires_grad_(True)
    for pm, ac in (("zeros", False), ("border", False)):
        assert torch.autograd.gradcheck(lambda v, l, a: multiscale_deformable_attention(v, shapes, l, a, pm, ac, query_mask=m),
                                        (value, loc, attn), eps=1e-6, atol=1e-6, rtol=1e-4)
    proj = torch.randn(B, Q, H, L, P, 3, generator=g, dtype=torch.float64) * 0.2
    ref = 0.3 + 0.4 * torch.rand(B, Q, L, 2, generator=g, dtype=torch.float64)
    proj.requires_grad_(True), ref.requires_grad_(True)
    out = fused_hf_module_core(value, shapes, proj, ref, "zeros", False, query_mask=m)
    g_v, g_p, g_r = torch.autograd.grad(out.sum(), (value, proj, ref))
    assert (g_p[~m] == 0).all() and (g_r[~m] == 0).all() and (out[~m] == 0).all() and g_p[m].abs().sum() > 0


# ------------------------------------------------------------------------------------------ containment
@pytest.mark.parametrize("poison", [float("nan"), float("inf"), -float("inf"), 1e30], ids=["nan", "pinf", "ninf", "1e30"])
def test_nothing_a_masked_query_holds_reaches_a_result(poison):
    value, shapes, loc, attn, go = _case(torch.float32)
    m = _qmask(value.shape[0], loc.shape[1])

    def op(v, l, a):
        return multiscale_deformable_attention(v, shapes, l, a, "zeros", False, query_mask=m)

    benign = _grads(op, (value, loc, attn), go)
    bad = [torch.where(_rows(t, m), t, torch.full_like(t, poison)) for t in (loc, attn, go)]
    for which in ((0,), (1,), (2,), (0, 1, 2)):
        l, a, g = (bad[i] if i in which else t for i, t in enumerate((loc, attn, go)))
        got = _grads(op, (value, l, a), g)
        for x, y in zip(got, benign):
            assert torch.isfinite(x).all() and torch.equal(x, y), which
    # ... and through the fused core: projection, reference points, grad_out
    value, shapes, proj, ref, go = _hf_inputs(4)
    m = _qmask(proj.shape[0], proj.shape[1], 1)

    def hf(v, p, r):
        return fused_hf_module_core(v, shapes, p, r, "border", True, query_mask=m)

    benign = _grads(hf, (value, proj, ref), go)
    got = _grads(hf, (value,) + tuple(torch.where(_rows(t, m), t, torch.full_like(t, poison)) for t in (proj, ref)),
                 torch.where(_rows(go, m), go, torch.full_like(go, poison)))
    for x, y in zip(got, benign):
        assert torch.isfinite(x).all() and torch.equal(x, y)


# ------------------------------------------------------------------------------------------ argument checks
def test_bad_masks_raise_value_error():
    value, shapes, loc, attn, _ = _case(torch.float32)
    B, Q = loc.shape[:2]
    hf = _hf_inputs(2, Q=Q)
    calls = (lambda mk: multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, query_mask=mk),
             lambda mk: fused_hf_module_core(*hf[:4], "zeros", False, query_mask=mk),
             lambda mk: apply_query_mask(loc, mk), lambda mk: functional.check_query_mask(mk, loc))
    for call in calls:
        with pytest.raises(ValueError, match="bool or uint8"):
            call(torch.ones(B, Q))                                  # float dtype
        with pytest.raises(ValueError, match="query_mask"):
            call(torch.ones(B, Q, 1, dtype=torch.bool))             # wrong rank
        with pytest.raises(ValueError, match="query_mask"):
            call(torch.ones(B, Q + 1, dtype=torch.bool))            # wrong shape
        with pytest.raises(ValueError, match="device"):
            call(torch.ones(B, Q, dtype=torch.bool, device="meta"))  # wrong device
    with pytest.raises(ValueError):
        functional.hip_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False,
                                                       query_mask=torch.ones(B, Q, dtype=torch.bool))  # host tensors


def test_a_bool_mask_travels_as_its_uint8_view_without_a_copy():
    m = _qmask(2, 9)
    u8 = functional.check_query_mask(m, torch.empty(2, 9, 3))
    assert u8.dtype == torch.uint8 and u8.data_ptr() == m.data_ptr()
    assert apply_query_mask(torch.ones(2, 9, 3), None) is not None


def test_sharded_operators_refuse_a_query_mask():
    from msda_triton_amd import distributed
    value, shapes, loc, attn, _ = _case(torch.float32)
    m = _qmask(value.shape[0], loc.shape[1])
    with pytest.raises(ValueError, match="query_mask"):
        distributed.sharded_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, query_mask=m)
    with pytest.raises(ValueError, match="query_mask"):
        distributed.row_sharded_multiscale_deformable_attention(value, shapes, loc, attn, "zeros", False, query_mask=m,
                                                                compute_only_as=(2, 0))


# ------------------------------------------------------------------------------------------ the C ABI
def test_qmasked_symbols_exist_for_every_suffix_with_the_masked_lists_plus_one_pointer():
    lib = _lib.load()
    assert _lib.has_query_mask()
    vp = ctypes.c_void_p
    for stem, twin, suffixes in (("msda_{}_qmasked_{}", "msda_{}_masked_{}", _lib.DTYPE_SUFFIXES),
                                 ("msda_{}_fused_levelref_qmasked_{}", "msda_{}_fused_levelref_masked_{}",
                                  _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES)):
        for suf in suffixes:
            for d in ("fwd", "bwd"):
                name = stem.format(d, suf)
                assert name in _lib.QUERY_MASK_SYMBOLS
                got, want = getattr(lib, name).argtypes, getattr(lib, twin.format(d, suf)).argtypes
                k = 2 if d == "fwd" else 3  # `query_mask` sits behind `value_mask`
                assert list(got) == list(want[:k]) + [vp] + list(want[k:]), name


def _qmasked_call(lib, host, family, suffix, d, vmask, qmask):
    """tests/test_value_mask._masked_call for the query-mask entry point of `family`"""
    backward, fused = family.startswith("bwd"), family.endswith("fused")
    fn = getattr(lib, ("msda_{}_fused_levelref_qmasked_{}" if fused else "msda_{}_qmasked_{}").format(family[:3], suffix))
    p = host.p
    B, I_, H, D, Q, S, stride = (d[k] for k in ("B", "I", "H", "D", "Q", "S", "stride"))
    sizes = (B, I_, H, D, Q, 1, S)
    gv = p if not fused else None
    if not backward:
        return fn(p, vmask, qmask, p, p, p, p, *sizes, 2, 0, 0, stride, None) if fused else fn(p, vmask, qmask, p, p, p, p, *sizes, 0, 0, stride, None)
    if fused:
        return fn(p, p, vmask, qmask, p, p, p, gv, p, p, *sizes, 2, 0, 0, 0, stride, None, 0, None)
    return fn(p, p, vmask, qmask, p, p, p, gv, p, p, *sizes, 0, 0, 0, stride, None, 0, None)


def test_a_null_mask_of_either_kind_is_a_bad_argument_before_any_pointer_is_read():
    import test_size_guards as sg
    lib = _lib.load()
    host = sg._Host()
    for family, suffixes in (("fwd", _lib.DTYPE_SUFFIXES), ("bwd", _lib.DTYPE_SUFFIXES),
                             ("fwd_fused", _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES),
                             ("bwd_fused", _lib.DTYPE_SUFFIXES + _lib.FUSED_STORAGE_SUFFIXES)):
        for suf in suffixes:
            for vm, qm, word in ((None, host.p, b"value_mask"), (host.p, None, b"query_mask"), (None, None, b"value_mask")):
                rc = _qmasked_call(lib, host, family, suf, sg._dims(I=4, D=4, Q=2, S=2), vm, qm)
                assert rc == -1, (family, suf, rc)
                assert word in lib.msda_last_error()
                # ... also where the sizes alone would be refused: the masks are looked at first
                assert _qmasked_call(lib, host, family, suf, sg._dims(I=1 << 24), vm, qm) == -1


def test_guards_answer_what_the_twins_answer():
    import test_size_guards as sg
    lib = _lib.load()
    for row in sg.ROWS:
        for family, suffix in (("fwd", "f32"), ("bwd", "f32"), ("bwd", "f64"), ("fwd_fused", "f32"), ("bwd_fused", "f32_sbf16")):
            if not sg._applies(row, family):
                continue
            es, ves = sg.SIZES[suffix]
            d = sg._isolates(row, family, es, ves)
            host = sg._Host()
            want = sg._call(lib, host, family, suffix, d)
            got = _qmasked_call(lib, host, family, suffix, d, host.p, host.p)
            assert got == want == sg.TOO_LARGE, (row, family, suffix, got, want, lib.msda_last_error())


# ------------------------------------------------------------------------------------------ the GPU file's mask generators
SHAPES = {"c2_like_f32": (2, 700, 4, 32, [(16, 16), (8, 8), (4, 4), (2, 2)], 4, 4),
          "bf16_g4": (2, 520, 4, 32, [(20, 17), (10, 9), (5, 4)], 4, 2),
          "d5_scalar": (2, 13, 3, 5, [(6, 4), (3, 2), (2, 5)], 3, 4),
          "one_element": (1, 300, 4, 64, [(16, 16), (8, 8), (4, 4)], 8, 2)}


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("kind", qmc.KINDS)
def test_each_mask_kind_masks_what_it_claims(kind, name):
    shape = SHAPES[name]
    B, Q = shape[:2]
    m = qmc.make_query_mask(kind, B, Q, 3, shape)
    assert m.shape == (B, Q) and m.dtype == torch.bool
    assert torch.equal(m, qmc.make_query_mask(kind, B, Q, 3, shape))  # seeded
    share = m.float().mean().item()
    if kind == "all_ones":
        assert m.all()
    else:
        assert share <= qmc.max_real_share(kind, B, Q), (kind, share)
    if kind == "bernoulli":
        assert 0.35 < share < 0.65 or B * Q < 100
    if kind == "tail":
        n = max(1, int(round(Q * qmc.TAIL_SHARE)))
        assert m[:B - 1].all() and m[B - 1, :Q - n].all() and not m[B - 1, Q - n:].any()
    if kind == "element0_masked":
        assert not m[0].any() and (B == 1 or m[1:].any())
    if kind == "all_zeros":
        assert not m.any()
    if kind == "one_real_query":
        assert int(m.sum()) == 1
    if kind == "slice_edges":
        bounds = qmc.slice_boundaries(*shape)
        assert bounds or Q < 8
        for b in bounds:
            for e in range(B):
                pol = e % 2 == 0
                # flips exactly at the boundary, one before and one after it
                want = [(b - 1, pol), (b, not pol), (b + 1, pol)]
                for q, v in want:
                    if 0 <= q < Q and not any(abs(q - b2) <= 1 for b2 in bounds if b2 != b):
                        assert bool(m[e, q]) == v, (b, e, q)


def test_slice_boundaries_follow_the_pipelines_constants():
    k = qmc.pipeline_constants()
    assert k["kWave"] == 64 and k["kWinMax"] == 64  # a wave, a gather window: what "64" means in the kernels' sources
    B, Q, H, D, levels, P, es = SHAPES["c2_like_f32"]
    L, n_pix = len(levels), sum(h * w for h, w in levels)
    bounds = qmc.slice_boundaries(B, Q, H, D, levels, P, es)
    G = qmc.unit_lanes(D, es)
    assert G == 8  # 32 fp32 channels in 16-byte pieces
    ns = qmc.cell_slices(B, n_pix, H, Q, L * P)
    assert ns == min(256 // (B * H), -(-Q * L * P // 2048), 9 * Q * L * P // (2 * n_pix), 64, Q) and ns > 1
    for b, why in ((k["kWave"] // G, "wave units"), (k["kBlock"] // G, "workgroup units"), (k["kBlockLds"] // G, "lds workgroup units"),
                   (-(-Q // ns), "query slice"), (k["kCellBlock"] // (L * P), "count trip"), (k["kPlaceBlock"] // P, "place round"),
                   (k["kPlaceBlockSmall"] // P, "small place round"), (k["kWinMax"] // P, "window / P")):
        assert b in bounds, (b, why, bounds)
    assert all(0 < b < Q for b in bounds)
    # 16-bit storage: twice the channels per 16-byte piece, half the lanes
    assert qmc.unit_lanes(32, 2) == 4 and qmc.unit_lanes(5, 4) == 8 and qmc.unit_lanes(64, 4) == 16


@pytest.mark.parametrize("kind", ["bernoulli", "tail", "slice_edges", "one_real_query", "all_zeros"])
@pytest.mark.parametrize("name", qmc.EXACT)
def test_exact_cases_stay_exact_under_a_query_mask(name, kind):
    """what the GPU file's exact grad_value test rests on: under the mask every sum is over a subset of the unmasked case's
    terms, so the bit budget does not grow and the float32 oracle still equals the float64 one"""
    qm = qmc.exact_query_mask(name, kind)
    for pm, ac in (("zeros", False), ("border", True)):
        s, ref = qmc.exact_reference(name, pm, ac, qm.numpy())
        masked = ~qm.numpy()
        assert (ref["out"][masked] == 0).all() and (ref["grad_attn"][masked] == 0).all() and (ref["grad_loc"][masked] == 0).all()
        if kind == "all_zeros":
            assert (ref["grad_value"] == 0).all()
