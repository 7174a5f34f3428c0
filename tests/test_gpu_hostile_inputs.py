"""GPU: hostile sampling inputs (tests/hostile_cases.py) through every launcher family, under the guarded allocation
rig.  DESIGN.md §5a states the contract; tests/test_hostile_cases.py shows on the CPU that it is the operation's.

  1. no store outside the call's buffers, and the call completes: every case runs under the rig (bands intact, the
     launcher's allocation count served) and is synchronised;
  2. FAR (finite) coordinates behave as the oracle says, at the tolerances of tests/test_gpu_parity.py;
  3. NONFINITE input is contained: the rows of every clean query, and grad_value of every batch element without a hostile
     query, equal the benign call's BIT FOR BIT — no assertion is made about the hostile rows;
  4. under "zeros" padding a sample with a non-finite coordinate and a finite weight adds nothing to grad_value.
Run with ``-m gpu``."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import hostile_cases as hc
from conftest import MODES, kink_mask
from guarded_alloc import GuardedAlloc, bits_equal
from msda_triton_amd import _lib, discrete, functional as F, ragged
from test_discrete_sampling import ref_discrete
from test_gpu_fused_ragged import SHAPES as FUSED_SHAPES
from test_gpu_parity import BWD_TOL, DEV, FWD_TOL
from test_gpu_value_mask import make_mask

pytestmark = pytest.mark.gpu

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
MODES2 = [("zeros", False), ("border", True)]
# test_hip_low_precision_vs_fp32_oracle_on_rounded_inputs' bounds
LOW_TOL = {F16: (2e-2, 2e-2), BF16: (4e-2, 2e-2)}


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


@functools.lru_cache(maxsize=None)
def oracle_lib():
    from oracle import msda_oracle
    msda_oracle.build()
    return msda_oracle


def rounded(c, storage):
    """the case as the kernels see it: every float tensor rounded to the storage type (in the arithmetic type's numpy)"""
    if storage in (F32, F64):
        return c
    return {k: (v if k == "shapes" else torch.from_numpy(v).to(storage).float().numpy()) for k, v in c.items()}


def reference(c, pm, ac, mask=None):
    """out, grad_value, grad_loc, grad_attn of the CPU oracle (float32 or float64 by the case's dtype); `mask`: [B, I] bool,
    the value-mask twins' semantics (padding pixels read zeros, their grad_value rows are zeros)"""
    o = oracle_lib()
    value = c["value"] if mask is None else np.where(mask[:, :, None, None], c["value"], 0).astype(c["value"].dtype)
    out = o.forward(value, c["shapes"], c["loc"], c["attn"], pm, ac)
    gv, gl, ga = o.backward(c["grad_out"], value, c["shapes"], c["loc"], c["attn"], pm, ac)
    if mask is not None:
        gv = np.where(mask[:, :, None, None], gv, 0)
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_attn=ga)


def rigged(call, n_alloc, what):
    """item 1: the call under the rig (pre-fill 0xFF), synchronised; bands intact and every allocation served"""
    with GuardedAlloc(0xFF, DEV) as rig:
        res = call()
    torch.cuda.synchronize()
    assert len(rig.served) == n_alloc, (what, rig.allocations)
    bad = rig.band_violations()
    assert not bad, (what, bad)
    return res


def to_dev(c, storage, value_storage=None):
    v, l, a, go = (torch.from_numpy(c[k]).to(DEV, storage) for k in ("value", "loc", "attn", "grad_out"))
    if value_storage is not None:  # (mixed storage: a 16-bit value pyramid next to float32 everything else)
        v = torch.from_numpy(c["value"]).to(DEV, value_storage)
    return v, torch.from_numpy(c["shapes"]).to(DEV), l, a, go


def run_plain(c, storage, pm, ac, what, mask=None, value_storage=None):
    v, s, l, a, go = to_dev(c, storage, value_storage)

    def call():
        out = F.msda_hip_fwd(v, s, l, a, pm, ac, value_mask=mask)
        return (out,) + F.msda_hip_bwd(go, v, s, l, a, pm, ac, value_mask=mask)

    res = rigged(call, 5, what)
    return dict(zip(("out", "grad_value", "grad_loc", "grad_attn"), res))


def assert_matches_oracle(got, ref, c, ac, storage, what, layout=None, tensors=("out", "grad_value", "grad_attn", "grad_loc")):
    """as test_gpu_parity.check_against_oracle (f32: kinks masked; f64: 1e-8, unmasked) and, for a tensor that comes back in
    16 bits, as test_hip_low_precision_vs_fp32_oracle_on_rounded_inputs.  `layout`: maps a [B, Q, H, L, P, 2] mask to the
    layout grad_loc has (per-level counts)."""
    layout = layout or (lambda m: m)
    for k in tensors:
        t, r = got[k], ref[k]
        assert bool(torch.isfinite(t).all()), (what, k)
        if t.dtype in LOW_TOL:
            atol, rtol = LOW_TOL[t.dtype]
            a, tol = t.float().cpu().numpy(), dict(atol=atol if k == "out" else atol * 4, rtol=rtol)
            if k == "grad_loc":
                keep = layout(~kink_mask(c["loc"], c["shapes"], ac, tol=2e-2))
                a, r = np.where(keep, a, 0), np.where(keep, r, 0)
                tol = dict(atol=atol * max(1.0, float(np.abs(ref[k]).max())), rtol=rtol * 2)
        else:
            a, tol = t.cpu().numpy(), (FWD_TOL if k == "out" else BWD_TOL)[t.dtype]
            if k == "grad_loc" and t.dtype == F32:
                keep = layout(~kink_mask(c["loc"], c["shapes"], ac))
                a, r = np.where(keep, a, 0), np.where(keep, r, 0)
        np.testing.assert_allclose(a, r, err_msg=f"{what} {k}", **tol)


def assert_contained(got, want, clean, what, per_query=("out", "grad_loc", "grad_attn"), per_batch=("grad_value",)):
    """item 3; `clean`: bool [Q], the clean queries of batch element 0 (every query of the other elements is clean)"""
    idx = torch.from_numpy(np.flatnonzero(clean)).to(DEV)
    for k in per_query:
        assert bits_equal(got[k][1:], want[k][1:]), f"{what}: {k} of a batch element without a hostile query changed"
        assert bits_equal(got[k][0][idx], want[k][0][idx]), f"{what}: {k} rows of clean queries of batch element 0 changed"
    for k in per_batch:
        assert bits_equal(got[k][1:], want[k][1:]), f"{what}: {k} of a batch element without a hostile query changed"


# ----------------------------------------------------------------------------------------- routes of the plain pair
R_DEFAULT = ("default", {}, {})
R_SORTED0 = ("sorted_records_in_ws", dict(value_path=2, records_in_grads=0), dict(value_path=2))
R_SORTED1 = ("sorted_records_in_grads", dict(value_path=2, records_in_grads=1), dict(value_path=2))
R_SINGLE = ("single_launch", dict(value_path=3), dict(value_path=1))
R_PASSES = ("two_passes_rounds_of_7", dict(value_path=2, ws_passes=2, q_round=7), dict(value_path=2, value_passes=2))
R_UNIT = ("unit_fwd", dict(unit_fwd=2), dict(fwd_variant=2))
R_PLAIN_FWD = ("no_lds_no_unit", dict(unit_fwd=0, lds_levels=0), dict(fwd_variant=0, sample_variant=0))
R_LDS1 = ("lds_one_plane", dict(unit_fwd=0, lds_levels=2, lds_planes=1), dict(fwd_variant=1, sample_variant=1, fwd_lds_planes=1))
R_LDS2 = ("lds_two_planes", dict(unit_fwd=0, lds_levels=2, lds_planes=2), dict(fwd_variant=1, sample_variant=1))
ALL_ROUTES = [R_DEFAULT, R_SORTED0, R_SORTED1, R_SINGLE, R_PASSES, R_UNIT, R_PLAIN_FWD, R_LDS1, R_LDS2]
ROUTES = {"d32_vec_g8": ALL_ROUTES, "c2_like_f32": ALL_ROUTES, "d5_scalar": [R_DEFAULT, R_SORTED1, R_SINGLE],
          "bf16_g4": [R_DEFAULT, R_SORTED1, R_SINGLE, R_UNIT], "fp16_d64": [R_DEFAULT, R_SORTED1, R_SINGLE, R_UNIT],
          "f64": [R_DEFAULT, R_SORTED0, R_SORTED1, R_SINGLE]}
PLAIN = [(n, r) for n, rs in ROUTES.items() for r in rs]
PLAIN_IDS = [f"{n}-{r[0]}" for n, r in PLAIN]


def confirm(route, what):
    info = _lib.last_launch_info()
    for k, v in route[2].items():
        assert info[k] == v, (what, k, info)


@pytest.mark.parametrize("name,route", PLAIN, ids=PLAIN_IDS)
def test_far_coordinates_behave_as_the_oracle_says(name, route):
    c, hq, storage = hc.plain_case(name)
    far = rounded(hc.far_case(c, hq, storage), storage)
    assert not hc.classify(far, storage).any()
    with options(**route[1]):
        for pm, ac in MODES:
            what = f"{name} {route[0]} {pm}/{ac}"
            got = run_plain(far, storage, pm, ac, what)
            confirm(route, what)
            assert_matches_oracle(got, reference(far, pm, ac), far, ac, storage, what)


NONFINITE_CASES = [(v, w) for w in ("loc", "attn") for v in hc.NONFINITE]


@pytest.mark.parametrize("name,route", PLAIN, ids=PLAIN_IDS)
def test_nonfinite_input_is_contained(name, route):
    c, hq, storage = hc.plain_case(name)
    cases = {f"{v}_{w}": hc.nonfinite_case(c, hq, hc.NONFINITE[v], w) for v, w in NONFINITE_CASES}
    # finite float32 inputs that turn non-finite inside the operation: +-Inf on the cast to float16 (the AMP case), or a pixel
    # coordinate that overflows float32 (+-3.0e38); with float64 arithmetic there is no such value
    over = hc.overflow_case(c, hq, storage)
    assert (over is None) == (storage == F64)
    if over is not None:
        cases["overflow"] = (over, None)
    clean = np.ones(c["loc"].shape[1], dtype=bool)
    clean[hq] = False
    with options(**route[1]):
        for pm, ac in MODES:
            benign = run_plain(c, storage, pm, ac, f"{name} {route[0]} {pm}/{ac} benign")
            confirm(route, name)
            for cname, (nf, planted) in cases.items():
                what = f"{name} {route[0]} {pm}/{ac} {cname}"
                assert hc.classify(nf, storage)[0][hq].all()
                got = run_plain(nf, storage, pm, ac, what)
                confirm(route, what)
                assert_contained(got, benign, clean, what)
                if pm == "zeros" and cname.endswith("_loc"):  # item 4, against the oracle on the neutralised case
                    neutral = rounded(hc.neutralised(nf, planted), storage)
                    r_gv = reference(neutral, pm, ac)["grad_value"]
                    gv = got["grad_value"]
                    assert bool(torch.isfinite(gv).all()), what
                    if storage in LOW_TOL:
                        atol, rtol = LOW_TOL[storage]
                        np.testing.assert_allclose(gv.float().cpu().numpy(), r_gv, atol=atol * 4, rtol=rtol, err_msg=what)
                    else:
                        np.testing.assert_allclose(gv.cpu().numpy(), r_gv, err_msg=what, **BWD_TOL[storage])


# ----------------------------------------------------------------------------------------- the value-mask twins
MASKED = [(n, r) for n in ("d32_vec_g8", "c2_like_f32") for r in (R_PLAIN_FWD, R_LDS2, R_SORTED1, R_SINGLE)] + \
         [("bf16_g4", R_DEFAULT), ("f64", R_DEFAULT)]


@pytest.mark.parametrize("name,route", MASKED, ids=[f"{n}-{r[0]}" for n, r in MASKED])
def test_masked_twins_on_hostile_inputs(name, route):
    """hostile coordinates clamp onto pixels whose mask byte is then read: pix[] must name a pixel of the level"""
    c, hq, storage = hc.plain_case(name)
    B, levels = c["value"].shape[0], [tuple(int(x) for x in hw) for hw in c["shapes"]]
    m = make_mask("bernoulli", B, levels, hc.seed_of("mask", name))
    m_dev, m_np = m.to(DEV), m.numpy()
    far = rounded(hc.far_case(c, hq, storage), storage)
    clean = np.ones(c["loc"].shape[1], dtype=bool)
    clean[hq] = False
    with options(**route[1]):
        for pm, ac in MODES2:
            what = f"{name} masked {route[0]} {pm}/{ac}"
            got = run_plain(far, storage, pm, ac, what, m_dev)
            confirm(route, what)
            assert_matches_oracle(got, reference(far, pm, ac, m_np), far, ac, storage, what)
            assert int(torch.count_nonzero(got["grad_value"][~m_dev])) == 0
            benign = run_plain(c, storage, pm, ac, what + " benign", m_dev)
            for v, w in NONFINITE_CASES:
                nf, _ = hc.nonfinite_case(c, hq, hc.NONFINITE[v], w)
                assert_contained(run_plain(nf, storage, pm, ac, f"{what} {v}_{w}", m_dev), benign, clean, f"{what} {v}_{w}")


# ----------------------------------------------------------------------------------------- mixed storage of the plain pair
@pytest.mark.parametrize("route", [R_LDS1, R_LDS2, R_SORTED1, R_SINGLE], ids=lambda r: r[0])
@pytest.mark.parametrize("vdt", [BF16, F16], ids=["f32_vbf16", "f32_vf16"])
def test_mixed_storage_on_hostile_inputs(vdt, route):
    """a 16-bit value pyramid (and grad_value) next to float32 sampling inputs: msda_*_f32_vbf16 / _vf16, which have the
    LDS-served variants; the value rounded to 16 bits is exact in float32, so out, grad_loc and grad_attn keep the float32
    bounds and grad_value, stored in 16 bits, the low-precision one"""
    c, hq, storage = hc.plain_case("c2_like_f32")
    c = dict(c, value=torch.from_numpy(c["value"]).to(vdt).float().numpy())
    far = hc.far_case(c, hq, storage)
    clean = np.ones(c["loc"].shape[1], dtype=bool)
    clean[hq] = False
    with options(**route[1]):
        for pm, ac in MODES2:
            what = f"mixed {vdt} {route[0]} {pm}/{ac}"
            got = run_plain(far, storage, pm, ac, what, value_storage=vdt)
            confirm(route, what)
            assert got["grad_value"].dtype == vdt and got["out"].dtype == F32
            assert_matches_oracle(got, reference(far, pm, ac), far, ac, storage, what)
            benign = run_plain(c, storage, pm, ac, what + " benign", value_storage=vdt)
            cases = [hc.nonfinite_case(c, hq, hc.NONFINITE[v], w)[0] for v, w in NONFINITE_CASES] + [hc.overflow_case(c, hq, storage)]
            for i, nf in enumerate(cases):
                assert_contained(run_plain(nf, storage, pm, ac, f"{what} case {i}", value_storage=vdt), benign, clean, f"{what} case {i}")


# ----------------------------------------------------------------------------------------- discrete sampling
DISCRETE = [(n, vp) for n in ("d32_vec_g8", "d5_scalar", "f64", "bf16_g4", "fp16_d64") for vp in (0, 2, 3)]


def run_discrete(c, storage, counts, what):
    v, s, l, a, go = to_dev(c, storage)
    B, Q, H = l.shape[:3]
    l, a = l.reshape(B, Q, H, -1, 2), a.reshape(B, Q, H, -1)

    def call():
        return (discrete.discrete_hip_fwd(v, s, l, a, counts),) + discrete.discrete_hip_bwd(go, v, s, l, a, counts)

    return dict(zip(("out", "grad_value", "grad_attn"), rigged(call, 4, what)))


@pytest.mark.parametrize("name,value_path", DISCRETE, ids=[f"{n}-value_path{vp}" for n, vp in DISCRETE])
def test_discrete_sampling_on_hostile_inputs(name, value_path):
    c, hq, storage = hc.plain_case(name)
    B, Q, H, L, P, _ = c["loc"].shape
    counts = (P,) * L
    levels = [tuple(int(x) for x in hw) for hw in c["shapes"]]
    clean = np.ones(Q, dtype=bool)
    clean[hq] = False
    far = rounded(hc.far_case(c, hq, storage), storage)
    with options(value_path=value_path):
        got = run_discrete(far, storage, counts, f"{name} discrete far")
        info = _lib.last_launch_info()
        assert info["fwd_variant"] == 3 and info["sample_variant"] == 2, info
        if value_path:
            assert info["value_path"] == (2 if value_path == 2 else 1), info
        # FAR: test_discrete_sampling.ref_discrete (the index in the coordinates' own precision, the sums in fp64)
        v64 = torch.from_numpy(far["value"]).double().requires_grad_(True)
        a64 = torch.from_numpy(far["attn"]).double().reshape(B, Q, H, L * P).requires_grad_(True)
        loc = torch.from_numpy(far["loc"]).reshape(B, Q, H, L * P, 2)
        r_out = ref_discrete(v64, levels, loc, a64, counts)
        r_gv, r_ga = torch.autograd.grad(r_out, [v64, a64], torch.from_numpy(far["grad_out"]).double())
        ref = dict(out=r_out.detach().numpy(), grad_value=r_gv.numpy(), grad_attn=r_ga.numpy())
        assert_matches_oracle(got, ref, far, False, storage, f"{name} discrete far", tensors=("out", "grad_value", "grad_attn"))
        benign = run_discrete(c, storage, counts, f"{name} discrete benign")
        for v, w in NONFINITE_CASES:
            nf, _ = hc.nonfinite_case(c, hq, hc.NONFINITE[v], w)
            what = f"{name} discrete {v}_{w}"
            assert_contained(run_discrete(nf, storage, counts, what), benign, clean, what, per_query=("out", "grad_attn"))


# ----------------------------------------------------------------------------------------- per-level counts, unfused
def to_ragged(c, counts):
    """the first counts[l] points of every level of a uniform case, level-major: loc [B, Q, H, S, 2], attn [B, Q, H, S]"""
    loc = np.concatenate([c["loc"][:, :, :, l, :n] for l, n in enumerate(counts)], axis=3)
    attn = np.concatenate([c["attn"][:, :, :, l, :n] for l, n in enumerate(counts)], axis=3)
    return loc, attn


def dropped_points_zeroed(c, counts):
    """the uniform case that computes the same: the points beyond counts[l] get weight 0 and an in-range location"""
    c = {k: v.copy() for k, v in c.items()}
    for l, n in enumerate(counts):
        c["attn"][:, :, :, l, n:] = 0
        c["loc"][:, :, :, l, n:] = 0.5
    return c


def run_ragged(c, storage, counts, pm, ac, what):
    v, s, _, _, go = to_dev(c, storage)
    loc, attn = to_ragged(c, counts)
    l, a = torch.from_numpy(loc).to(DEV, storage), torch.from_numpy(attn).to(DEV, storage)

    def call():
        return (ragged.ragged_hip_fwd(v, s, l, a, pm, ac, counts),) + ragged.ragged_hip_bwd(go, v, s, l, a, pm, ac, counts)

    return dict(zip(("out", "grad_value", "grad_loc", "grad_attn"), rigged(call, 5, what)))


@pytest.mark.parametrize("value_path", [0, 2, 3])
@pytest.mark.parametrize("name,counts", [("d32_vec_g8", (3, 4, 2, 1)), ("d5_scalar", (1, 3, 2)), ("bf16_g4", (3, 4, 2)),
                                         ("fp16_d64", (5, 8, 2)), ("f64", (2, 3))])
def test_per_level_counts_on_hostile_inputs(name, counts, value_path):
    c, hq, storage = hc.plain_case(name)
    clean = np.ones(c["loc"].shape[1], dtype=bool)
    clean[hq] = False
    far = rounded(hc.far_case(c, hq, storage), storage)
    with options(value_path=value_path):
        for pm, ac in MODES2:
            what = f"{name} ragged {counts} {pm}/{ac}"
            got = run_ragged(far, storage, counts, pm, ac, what)
            if value_path:
                assert _lib.last_launch_info()["value_path"] == (2 if value_path == 2 else 1)
            zeroed = dropped_points_zeroed(far, counts)
            ref = reference(zeroed, pm, ac)
            ref["grad_loc"], ref["grad_attn"] = to_ragged(dict(loc=ref["grad_loc"], attn=ref["grad_attn"]), counts)
            assert_matches_oracle(got, ref, far, ac, storage, what,
                                  layout=lambda m: to_ragged(dict(loc=m, attn=far["attn"]), counts)[0])
            benign = run_ragged(c, storage, counts, pm, ac, what + " benign")
            for v, w in NONFINITE_CASES:
                nf, _ = hc.nonfinite_case(c, hq, hc.NONFINITE[v], w)
                assert_contained(run_ragged(nf, storage, counts, pm, ac, f"{what} {v}_{w}"), benign, clean, f"{what} {v}_{w}")


# ----------------------------------------------------------------------------------------- the fused families
FUSED_STORAGE = {"f32": (F32, F32), "f64": (F64, F64), "fp16": (F16, F16), "bf16": (BF16, BF16), "sbf16": (BF16, F32),
                 "sf16": (F16, F32)}
FUSED_COUNTS = (3, 6, 3)
FAMILIES = ["uniform", "levelref", "levelref_masked", "ragged_fused", "hf_box_fused"]


def fused_case(family, ref_dim):
    """float64 host tensors: one shape per family — test_gpu_fused_ragged's d32 with three levels; counts [3, 6, 3] for the
    per-level-count families, P = 4 for the uniform ones"""
    B, Q, H, D, levels = FUSED_SHAPES["d32"]
    levels = levels[:len(FUSED_COUNTS)]
    g = torch.Generator().manual_seed(hc.seed_of("fused", family, ref_dim))
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g)
    if family in ("ragged_fused", "hf_box_fused"):
        proj = torch.randn(B, Q, H, sum(FUSED_COUNTS), 3, generator=g) * 1.5
    else:
        proj = torch.randn(B, Q, H, len(levels), 4, 3, generator=g) * 1.5
    if family == "hf_box_fused":
        ref_dim = 4
    ref = torch.rand(*((B, Q, len(levels), ref_dim) if family.startswith("levelref") else (B, Q, ref_dim)), generator=g)
    gout = torch.rand(B, Q, H, D, generator=g)
    mask = make_mask("bernoulli", B, levels, 5) if family == "levelref_masked" else None
    return dict(value=value, shapes=torch.tensor(levels), proj=proj, ref=ref, gout=gout, mask=mask, levels=levels)


def run_fused(family, t, proj, ref, storage, pm, ac, what):
    sdt, rdt = FUSED_STORAGE[storage]
    v, pr, go = (x.to(DEV, sdt) for x in (t["value"], proj, t["gout"]))
    s, rf = t["shapes"].to(DEV), ref.to(DEV, rdt)
    mask = t["mask"].to(DEV) if t["mask"] is not None else None
    if family == "ragged_fused":
        fwd = lambda: ragged.ragged_hip_fwd_fused(v, s, pr, rf, pm, ac, FUSED_COUNTS)  # noqa: E731
        bwd = lambda: ragged.ragged_hip_bwd_fused(go, v, s, pr, rf, pm, ac, FUSED_COUNTS)  # noqa: E731
    elif family == "hf_box_fused":
        fwd = lambda: ragged.hf_box_hip_fwd_fused(v, s, pr, rf, pm, ac, FUSED_COUNTS)  # noqa: E731
        bwd = lambda: ragged.hf_box_hip_bwd_fused(go, v, s, pr, rf, pm, ac, FUSED_COUNTS)  # noqa: E731
    else:
        kw = dict(levelref=True, value_mask=mask) if family.startswith("levelref") else {}
        fwd = lambda: F.msda_hip_fwd_fused(v, s, pr, rf, pm, ac, **kw)  # noqa: E731
        bwd = lambda: F.msda_hip_bwd_fused(go, v, s, pr, rf, pm, ac, **kw)  # noqa: E731

    def call():
        out, grads = fwd(), bwd()
        assert out is not None and grads is not None, what
        return (out,) + tuple(grads)

    return dict(zip(("out", "grad_value", "grad_proj", "grad_ref"), rigged(call, 5, what)))


def prologue(family, proj, shapes, ref):
    if family == "uniform":
        return F.module_sampling_inputs(proj, shapes, ref)
    if family.startswith("levelref"):
        return F.hf_module_sampling_inputs(proj, shapes, ref)
    if family == "ragged_fused":
        return ragged.ragged_module_sampling_inputs(proj, shapes, ref, FUSED_COUNTS)
    return F.hf_box_sampling_inputs(proj, ref, FUSED_COUNTS)


def fused_reference(family, t, proj, ref, pm, ac, kink_tol=1e-4):
    """fp64 on the host: the family's prologue in PyTorch, the oracle on its points and weights (per-level counts as a
    uniform case whose padding points carry weight 0), autograd through the prologue for grad_proj and grad_ref.
    -> (reference dict, keep masks for grad_proj [.., 3] and grad_ref's queries [B, Q])"""
    proj64, ref64 = proj.double().requires_grad_(True), ref.double().requires_grad_(True)
    pts, att = prologue(family, proj64, t["shapes"], ref64)
    B, Q, H = pts.shape[:3]
    ragged_layout = pts.dim() == 5
    L = len(t["levels"])
    if ragged_layout:
        P = max(FUSED_COUNTS)
        loc = np.full((B, Q, H, L, P, 2), 0.5)
        attn = np.zeros((B, Q, H, L, P))
        s0 = 0
        for l, n in enumerate(FUSED_COUNTS):
            loc[:, :, :, l, :n] = pts.detach().numpy()[:, :, :, s0:s0 + n]
            attn[:, :, :, l, :n] = att.detach().numpy()[:, :, :, s0:s0 + n]
            s0 += n
    else:
        loc, attn = pts.detach().numpy(), att.detach().numpy()
    assert np.isfinite(loc).all() and np.isfinite(attn).all()
    c = dict(value=t["value"].double().numpy(), shapes=t["shapes"].numpy(), loc=loc, attn=attn, grad_out=t["gout"].double().numpy())
    r = reference(c, pm, ac, t["mask"].numpy() if t["mask"] is not None else None)
    kink = kink_mask(loc, c["shapes"], ac, tol=kink_tol)
    gl, ga = r["grad_loc"], r["grad_attn"]
    if ragged_layout:
        gl, ga = to_ragged(dict(loc=gl, attn=ga), FUSED_COUNTS)
        kink, _ = to_ragged(dict(loc=kink, attn=attn), FUSED_COUNTS)
    g_proj, g_ref = torch.autograd.grad([pts, att], [proj64, ref64], [torch.from_numpy(np.ascontiguousarray(gl)),
                                                                       torch.from_numpy(np.ascontiguousarray(ga))])
    keep_proj = np.ones(tuple(proj.shape), dtype=bool)
    keep_proj[..., :2] = ~kink.reshape(tuple(proj.shape[:-1]) + (2,))
    keep_ref = ~kink.reshape(B, Q, -1).any(-1)
    return dict(out=r["out"], grad_value=r["grad_value"], grad_proj=g_proj.numpy(), grad_ref=g_ref.numpy()), keep_proj, keep_ref


def masked(keep, a, b):
    keep = keep.reshape(keep.shape + (1,) * (a.ndim - keep.ndim)) if keep.ndim < a.ndim else keep
    return np.where(keep, a, 0), np.where(keep, b, 0)


@pytest.mark.parametrize("where", ["offset", "logit", "ref"])
@pytest.mark.parametrize("storage", list(FUSED_STORAGE))
@pytest.mark.parametrize("family", FAMILIES)
def test_fused_families_far_inputs_behave_as_the_reference_says(family, storage, where):
    """Every fused kernel instantiation — f32, f64, pure fp16 / bf16, and the module's 16-bit storage next to float32
    reference points — against the fp64 reference on the inputs as they are STORED.  f32 / f64: the bounds of
    tests/test_gpu_parity.py.  A tensor that comes back in 16 bits: those of
    test_hip_low_precision_vs_fp32_oracle_on_rounded_inputs — out (atol, rtol), grad_value atol * 4, and for grad_proj and
    grad_ref, which carry grad_loc through the prologue's chain rule, grad_loc's: atol * max(1, largest reference entry),
    rtol * 2, offsets within 2e-2 of a kink masked.  grad_ref sums a query's samples, so a query is compared when none of
    its samples sits within 1e-4 of a kink (the kernels form the coordinate in float32 from the stored values in every
    storage type, as the f32 case does; at 2e-2 no query would be left)."""
    sdt, rdt = FUSED_STORAGE[storage]
    for (pm, ac), ref_dim in zip(MODES2, (2, 4)):
        t = fused_case(family, ref_dim)
        Q = t["proj"].shape[1]
        hq = hc.hostile_queries(Q, hc.seed_of("fused hq", family))
        values = hc.fused_far_values(rdt if where == "ref" else sdt)
        proj, ref = hc.plant_fused(t["proj"].double(), t["ref"].double(), hq, values, where)
        # (the inputs as the kernels see them: rounded to their storage before the fp64 reference reads them)
        proj, ref = proj.to(sdt).double(), ref.to(rdt).double()
        assert bool(torch.isfinite(proj).all()) and bool(torch.isfinite(ref).all())
        t = dict(t, value=t["value"].to(sdt).double(), gout=t["gout"].to(sdt).double())
        what = f"{family} {storage} far {where} {pm}/{ac}"
        res = run_fused(family, t, proj, ref, storage, pm, ac, what)
        want, keep_proj, keep_ref = fused_reference(family, t, proj, ref, pm, ac)
        if storage == "f64":
            keep_proj, keep_ref = np.ones_like(keep_proj), np.ones_like(keep_ref)  # (as the f64 parity tests: no kink mask)
        elif sdt in LOW_TOL:
            keep_proj = fused_reference(family, t, proj, ref, pm, ac, kink_tol=2e-2)[1]
        for k, keep in (("out", None), ("grad_value", None), ("grad_proj", keep_proj), ("grad_ref", keep_ref)):
            g, r = res[k], want[k]
            a = g.double().cpu().numpy()
            if g.dtype in LOW_TOL:
                atol, rtol = LOW_TOL[g.dtype]
                tol = dict(atol=atol, rtol=rtol) if k == "out" else dict(atol=atol * 4, rtol=rtol) if k == "grad_value" else \
                    dict(atol=atol * max(1.0, float(np.abs(r).max())), rtol=rtol * 2)
                # the chain rule multiplies grad_loc by the offset (65504 in float16, for a box narrow enough to keep that
                # sample in range): where the TRUE gradient is at the edge of the storage type's range or beyond it, no
                # finite value of the type is right — the result there may be an infinity, or the NaN that per-head
                # partials overflowing with both signs sum to.  Everywhere else it must be finite and within the bound.
                edge = np.abs(r) > 0.9 * torch.finfo(g.dtype).max
                a, r = np.where(edge & ~np.isfinite(a), 0, a), np.where(edge & ~np.isfinite(a), 0, r)
            else:
                tol = (FWD_TOL if k == "out" else BWD_TOL)[g.dtype]
            assert np.isfinite(a).all(), (what, k)
            if keep is not None:
                a, r = masked(keep, a, r)
            np.testing.assert_allclose(a, r, err_msg=f"{what} {k}", **tol)


@pytest.mark.parametrize("storage", list(FUSED_STORAGE))
@pytest.mark.parametrize("family", FAMILIES)
def test_fused_families_contain_nonfinite_input(family, storage):
    """NaN / +-Inf in a query's offsets, logits or reference point, and the finite values that turn non-finite inside the
    call: +-Inf in a 16-bit projection (the AMP case), a pixel coordinate beyond float32 (+-3.0e38)"""
    sdt, rdt = FUSED_STORAGE[storage]
    for (pm, ac), ref_dim in zip(MODES2, (2, 4)):
        t = fused_case(family, ref_dim)
        Q = t["proj"].shape[1]
        hq = hc.hostile_queries(Q, hc.seed_of("fused hq", family))
        clean = np.ones(Q, dtype=bool)
        clean[hq] = False
        benign = run_fused(family, t, t["proj"], t["ref"], storage, pm, ac, f"{family} {storage} benign")
        for k, v in benign.items():
            assert bool(torch.isfinite(v).all()), (family, storage, k)
        value_sets = {v: [x] for v, x in hc.NONFINITE.items()}
        value_sets["overflow"] = None  # finite inputs that turn non-finite in the tensor's storage or the arithmetic type
        for vname, values in value_sets.items():
            for where in ("offset", "logit", "ref"):
                if values is None:
                    values_here = hc.fused_far_values(rdt if where == "ref" else sdt, overflowing=True)
                    if not values_here:
                        continue  # (float64: every value stays far)
                else:
                    values_here = values
                what = f"{family} {storage} {pm}/{ac} {vname} in {where}"
                proj, ref = hc.plant_fused(t["proj"], t["ref"], hq, values_here, where)
                got = run_fused(family, t, proj, ref, storage, pm, ac, what)
                assert_contained(got, benign, clean, what, per_query=("out", "grad_proj", "grad_ref"))
