"""Every kernel that maps a workgroup to a (plane, slot) under the FLAT 1-D grid of `plane_grid` (msda_launch.hpp), whose
block index `decode_block` (msda_common.hpp) takes apart with `bid & 7`, `t % slots`, `t / slots` and whose padding
blocks return early — reached only with more than 65 535 planes, groups of eight planes, or slots, at real sizes.
tests/geometry_cases.py holds the cases and what makes them reach the form; tests/test_geometry_cases.py their
preconditions.  Run with ``-m gpu``.

Every run takes the difference of the launch counters "grid_xcd3d_launches" / "grid_linear2d_launches" /
"grid_flat_launches" (msda_last_launch_info) around the call: the flat counter must rise by exactly the plane_grid
launches of the route, the others must not move (P4: by exactly the passes that have few slots).  Every comparison is
an equality on exactly representable inputs — with the fp64 oracle rounded once, or bit for bit with the same call cut
into parts small enough for a 3-D / 2-D grid — except where the fused prologue's softmax is involved, which takes
tests/test_gpu_fused_ragged.assert_fp32_close, the suite's bound for it."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import geometry_cases as gc
import large_cases as lc
from geometry_cases import FLAT, LINEAR2D, XCD3D
from large_cases import DEV

pytestmark = pytest.mark.gpu
BASE = dict(unit_fwd=0, lds_levels=0)  # the 256-thread gather kernels unless a route says otherwise


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


@contextlib.contextmanager
def counted(expect, what):
    """Asserts that the launches inside moved the grid-form counters by exactly `expect` ({form: launches}, others 0)."""
    before = launch_info()
    yield
    torch.cuda.synchronize()
    after = launch_info()
    got = {k: after[k] - before[k] for k in gc.FORMS}
    want = {k: expect.get(k, 0) for k in gc.FORMS}
    print(f"{what}: grid forms {got}")
    assert got == want, f"{what}: grid-form launches {got}, expected {want}"


@pytest.fixture(autouse=True)
def _free_device_memory(request):
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    print(f"PEAK {request.node.name} {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    torch.cuda.empty_cache()


def _drop_cached_inputs():
    _inputs.cache_clear()
    reference.cache_clear()
    _p4_reference.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_inputs_at_the_end():
    yield
    _drop_cached_inputs()


def _shapes(levels):
    return torch.tensor(levels, dtype=torch.int64, device=DEV)


# ----------------------------------------------------------------------------------------- shared inputs and references
_held = []  # whose tensors are cached: one case at a time, so that a test holds what ITS case needs


def inputs(name, D, kind):
    """The case's tensors on the device (made once per case, read-only, dropped when the next case begins; the gigabyte
    tensors of P3 are dropped with every test)."""
    key = (name, D, kind) if name == "P3" else (name,)
    if _held != [key]:
        _drop_cached_inputs()
        _held[:] = [key]
    return _inputs(name, D, kind)


@functools.lru_cache(maxsize=None)
def _inputs(name, D, kind):
    need = gc.device_bytes(name, D, kind, dict(value_path=2))[0]
    assert need < gc.MEMORY_LIMIT, (name, D, kind, need)
    lc.claim_memory(need, f"{name} D={D} {kind}")
    return gc.build(name, D, kind, DEV)


@functools.lru_cache(maxsize=None)
def reference(name, D, kind, pm, ac):
    """The fp64 oracle on the WHOLE tensors of a P1 / P2 case (computed once per mode, shared by the routes); asserts that
    the float32 oracle reproduces it bitwise, so a correct float32 kernel must equal it."""
    t = inputs(name, D, kind)
    c = gc.as_case(t, name)
    if kind == "masked":
        c = gc.apply_mask(c, t["mask"])
    ref, exact = gc.discrete_all(c) if kind == "discrete" else gc.oracle_all(c, pm, ac)
    assert exact, f"{name} D={D} {kind} {pm} {ac}: the fixture is not exact in float32"
    if kind == "masked":  # the rows of padding pixels take no gradient
        ref["grad_value"] = np.where(t["mask"].cpu().numpy().astype(bool)[:, :, None, None], ref["grad_value"], 0.0)
    return ref


def run_operator(t, pm, ac, needs, value=None, sel=None):
    """The operator through the public API on the built tensors (queries `sel` only); -> {tensor name: result}."""
    from msda_triton_amd import multiscale_deformable_attention
    q = slice(None) if sel is None else sel
    discrete = t.get("discrete", False)
    v = (t["value"] if value is None else value).detach().requires_grad_(needs[0])
    l = t["loc"][:, q].detach().requires_grad_(needs[1] and not discrete)
    a = t["attn"][:, q].detach().requires_grad_(needs[2])
    kw = {}
    if "counts" in t:
        kw["points_per_level"] = t["counts"]
    if discrete:
        kw["sampling_mode"] = "discrete"
    if "mask" in t:
        kw["value_mask"] = t["mask"]
    out = multiscale_deformable_attention(v, _shapes(t["levels"]), l, a, pm, ac, **kw)
    if any(needs):
        out.backward(t["grad_out"][:, q])
    torch.cuda.synchronize()
    got = dict(out=out.detach())
    for k, x in (("grad_value", v), ("grad_loc", l), ("grad_attn", a)):
        if x.requires_grad:
            got[k] = x.grad
    return got


def assert_equal_reference(got, ref, what):
    for k, x in got.items():
        lc.assert_matches(x, ref[k], True, f"{what} {k}", forward=k == "out")


# =========================================================================================================
# P1 / P2: more planes than a grid dimension holds — every kernel family, every route
# =========================================================================================================
# route: kind of input, options on top of BASE, which gradients, plane_grid launches, what last_launch_info must say, head dims
ALL, SAMPLE = (True, True, True), (False, True, True)
ROUTES = {
    # forward + sample gradients, the 256-thread kernels (value frozen: no grad_value pass)
    "general": ("bilinear", {}, SAMPLE, 2, dict(fwd_variant=0, sample_variant=0), (4, 3)),
    # ... and their variants that serve the coarse levels from LDS, one plane per 1024-thread workgroup (16-byte pieces only)
    "lds_levels": ("bilinear", dict(lds_levels=2, lds_planes=1), SAMPLE, 2,
                   dict(fwd_variant=1, fwd_lds_planes=1, sample_variant=1), (4,)),
    # + the single-launch grad_value kernel
    "single_launch": ("bilinear", dict(value_path=3), ALL, 3, dict(fwd_variant=0, sample_variant=0, value_path=1), (4, 3)),
    # + the sorted pipeline: count, (scan,) level-major place, gather, finish
    "sorted": ("bilinear", dict(value_path=2), ALL, 6, dict(value_path=2, value_passes=1), (4, 3)),
    # ... with the plane-major place pass, which shares the count pass's grid
    "plane_major_place": ("bilinear", dict(value_path=2, place_path=1, strict=0), ALL, 5, dict(value_path=2), (4, 3)),
    # the value-mask twins, the masked finish pass among them; NaN in the padding pixels
    "value_mask": ("masked", dict(value_path=2), ALL, 6, dict(fwd_variant=0, sample_variant=0, value_path=2), (4, 3)),
    "points_per_level": ("ragged", {}, ALL, 3, dict(fwd_variant=0, sample_variant=0, value_path=1), (4, 3)),
    "discrete": ("discrete", {}, ALL, 3, dict(fwd_variant=3, sample_variant=2, value_path=1), (4, 3)),
}
PLANE_RUNS = [(n, r, D) for n in ("P1", "P2") for r, spec in ROUTES.items() for D in spec[5]]


@pytest.mark.parametrize("name,route,D", PLANE_RUNS, ids=[f"{n}-{r}-D{D}" for n, r, D in PLANE_RUNS])
def test_many_planes_take_the_flat_grid(name, route, D):
    kind, opts, needs, launches, info, _ = ROUTES[route]
    t = dict(inputs(name, D, kind), discrete=kind == "discrete")
    value = None
    if kind == "masked":  # whatever the padding pixels hold must not reach a register
        value = torch.where(t["mask"][:, :, None, None] != 0, t["value"], torch.full_like(t["value"], float("nan")))
    modes = [("border", False)] if kind == "discrete" else gc.modes_for(name, kind)
    with options(**{**BASE, **gc.CASES[name]["options"], **opts}):
        for pm, ac in modes:
            ref = reference(name, D, kind, pm, ac)
            with counted({FLAT: launches}, f"{name} {route} D={D} {pm} {ac}"):
                got = run_operator(t, pm, ac, needs, value)
            got_info = launch_info()
            assert {k: got_info[k] for k in info} == info, (route, got_info)
            assert set(got) == {"out"} | {k for k, n in zip(("grad_value", "grad_loc", "grad_attn"), needs)
                                         if n and not (kind == "discrete" and k == "grad_loc")}
            assert_equal_reference(got, ref, f"{name} {route} D={D} {pm} {ac}")


@pytest.mark.parametrize("name", ["P1x2", "P2x2"])
def test_two_planes_per_workgroup_take_the_flat_grid(name):
    """The LDS-served forward with the planes of two neighbouring heads per workgroup halves the plane count, so these
    shapes have twice the planes of P1 / P2.  Forward only: the sample-gradient kernel has no such variant."""
    t = inputs(name, 4, "bilinear")
    with options(**{**BASE, **gc.CASES[name]["options"], **dict(lds_levels=2, lds_planes=2)}):
        for pm, ac in gc.modes_for(name):
            ref = reference(name, 4, "bilinear", pm, ac)
            with counted({FLAT: 1}, f"{name} {pm} {ac}"):
                got = run_operator(t, pm, ac, (False, False, False))
            info = launch_info()
            assert info["fwd_variant"] == 1 and info["fwd_lds_planes"] == 2, info
            assert info["fwd_workgroups"] >= gc.CASES[name]["B"] * gc.CASES[name]["H"] // 2
            assert_equal_reference(got, ref, f"{name} {pm} {ac}")


# ----------------------------------------------------------------------------------------- the fused module core
def run_fused(value, levels, proj, ref, go, pm, ac, fused=True, need_value=True):
    """-> (out, grad_value | None, grad_proj, grad_ref) of fused_module_core, or of the prologue in PyTorch around the operator."""
    from msda_triton_amd import multiscale_deformable_attention
    from msda_triton_amd.functional import fused_module_core, module_sampling_inputs
    v = value.detach().requires_grad_(need_value)
    pr, rf = proj.detach().requires_grad_(True), ref.detach().requires_grad_(True)
    shapes = _shapes(levels)
    if fused:
        out = fused_module_core(v, shapes, pr, rf, pm, ac)
    else:
        out = multiscale_deformable_attention(v, shapes, *module_sampling_inputs(pr, shapes, rf), pm, ac)
    out.backward(go)
    torch.cuda.synchronize()
    return out.detach(), v.grad, pr.grad, rf.grad


@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("name", ["P1", "P2"])
def test_fused_module_core_with_many_planes(name, D):
    """The softmax is not exact, so the reference is the same call on two batch halves, whose grids the counters show to
    be 3-D / 2-D: out, grad_proj and grad_ref bit for bit; grad_value within the suite's fused bound of that call and of
    the unfused composition."""
    from test_gpu_fused_ragged import assert_fp32_close
    t = inputs(name, D, "fused")
    B, levels = gc.CASES[name]["B"], t["levels"]
    pm, ac = gc.modes_for(name, "fused")[0]
    with options(**{**BASE, **gc.CASES[name]["options"]}):
        with counted({FLAT: 3}, f"{name} fused D={D}"):  # forward, backward prologue + sample half, single-launch grad_value
            out, gv, gp, gr = run_fused(t["value"], levels, t["proj"], t["ref"], t["grad_out"], pm, ac)
        info = launch_info()
        assert info["fwd_variant"] == 0 and info["sample_variant"] == 0 and info["value_path"] == 1, info
        half = (B + 1) // 2
        for b0, b1 in ((0, half), (half, B)):
            with counted({gc.split_form(name): 3}, f"{name} fused D={D} batch elements {b0}..{b1}"):
                part = run_fused(t["value"][b0:b1], levels, t["proj"][b0:b1], t["ref"][b0:b1], t["grad_out"][b0:b1], pm, ac)
            for k, whole, p in zip(("out", "grad_value", "grad_proj", "grad_ref"), (out, gv, gp, gr), part):
                if k != "grad_value":
                    assert torch.equal(whole[b0:b1], p), f"{name} D={D} {k} differs from the call on batch elements {b0}..{b1}"
            assert_fp32_close((out[b0:b1], gv[b0:b1]), (part[0], part[1]))
        unfused = run_fused(t["value"], levels, t["proj"], t["ref"], t["grad_out"], pm, ac, fused=False)
        assert_fp32_close((out, gv), (unfused[0], unfused[1]))


# =========================================================================================================
# P3: 65 537 slots on seven planes (XCD order, one padding plane)
# =========================================================================================================
def _halves(Q):
    return (slice(0, Q // 2), slice(Q // 2, Q))


def _p3_mode(D):
    return gc.MODES[D % 2]


@pytest.mark.parametrize("D", [33, 132])
@pytest.mark.parametrize("route", ["bilinear", "discrete"])
def test_many_slots_take_the_flat_grid(route, D):
    """Forward and sample gradients (discrete: the attention-weight gradient) with `value` frozen.  Whole tensors: bit
    for bit the same call on two query halves (3-D grids).  Oracle: equality on the queries a truncated or mis-decoded
    slot would move (geometry_cases.p3_queries)."""
    t = dict(inputs("P3", D, route), discrete=route == "discrete")
    Q = gc.CASES["P3"]["Q"]
    pm, ac = ("border", False) if route == "discrete" else _p3_mode(D)
    with counted({FLAT: 2}, f"P3 {route} D={D}"):
        got = run_operator(t, pm, ac, SAMPLE)
    info = launch_info()
    assert (info["fwd_variant"], info["sample_variant"]) == ((3, 2) if route == "discrete" else (0, 0)), info
    assert info["fwd_workgroups"] == 8 * (gc.GRID_LIMIT + 2)  # eight plane columns (one of padding) x 65 537 slots
    for sel in _halves(Q):
        with counted({XCD3D: 2}, f"P3 {route} D={D} queries {sel.start}..{sel.stop}"):
            part = run_operator(t, pm, ac, SAMPLE, sel=sel)
        assert set(part) == set(got)
        for k in got:
            assert torch.equal(got[k][:, sel], part[k]), f"P3 {route} D={D}: {k} differs from the call on queries {sel.start}..{sel.stop}"
        del part
    qs = gc.p3_queries(D)
    c = gc.as_case(t, "P3", qs)
    ref, exact = gc.discrete_all(c) if route == "discrete" else gc.oracle_all(c, pm, ac)
    assert exact, "the compared queries are not exact in float32"
    q = torch.tensor(qs, device=DEV)
    assert_equal_reference({k: x[:, q] for k, x in got.items()}, ref, f"P3 {route} D={D}")


@pytest.mark.parametrize("D", [33, 132])
def test_fused_module_core_with_many_slots(D):
    """fused_module_core forward, grad_proj and grad_ref (value frozen): bit for bit the call on two query halves; on
    the compared queries within the fused bound of the unfused composition."""
    from test_gpu_fused_ragged import assert_fp32_close
    t = inputs("P3", D, "fused")
    Q, levels = gc.CASES["P3"]["Q"], t["levels"]
    pm, ac = _p3_mode(D)
    with counted({FLAT: 2}, f"P3 fused D={D}"):
        out, gv, gp, gr = run_fused(t["value"], levels, t["proj"], t["ref"], t["grad_out"], pm, ac, need_value=False)
    assert gv is None
    for sel in _halves(Q):
        with counted({XCD3D: 2}, f"P3 fused D={D} queries {sel.start}..{sel.stop}"):
            part = run_fused(t["value"], levels, t["proj"][:, sel], t["ref"][:, sel], t["grad_out"][:, sel], pm, ac, need_value=False)
        for k, whole, p in zip(("out", "grad_proj", "grad_ref"), (out, gp, gr), (part[0], part[2], part[3])):
            assert torch.equal(whole[:, sel], p), f"P3 fused D={D}: {k} differs from the call on queries {sel.start}..{sel.stop}"
        del part
    q = torch.tensor(gc.p3_queries(D), device=DEV)
    want = run_fused(t["value"], levels, t["proj"][:, q], t["ref"][:, q], t["grad_out"][:, q], pm, ac, fused=False, need_value=False)
    assert_fp32_close((out[:, q], gp[:, q], gr[:, q]), (want[0], want[2], want[3]))


# =========================================================================================================
# P4: the finish pass with 65 536 slots
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def _p4_reference():
    """Per head: (pixels with a gradient, their fp64 grad_value rows), the oracle one head at a time (heads are
    independent; grad_value does not depend on `value`, so the plain and the masked test share it)."""
    t = inputs("P4", 4, "bilinear")
    c = gc.as_case(t, "P4")
    pm, ac = gc.P4_MODE
    rows = []
    for h in range(gc.CASES["P4"]["H"]):
        ref, exact = gc.oracle_all(gc.head_case(c, h), pm, ac)
        assert exact, f"P4 head {h}: the fixture is not exact in float32"
        gv = ref["grad_value"].reshape(-1, ref["grad_value"].shape[-1])
        nz = np.flatnonzero(np.abs(gv).max(axis=1) > 0)
        rows.append((torch.from_numpy(nz), torch.from_numpy(gv[nz]).to(torch.float32)))
    return rows


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "value_mask"])
def test_finish_pass_with_65536_slots(masked):
    """One level of 2047 x 2049 pixels, seven planes: the finish pass (64 pixels per workgroup) is the only launch with a
    flat grid; count, place and gather have a few slots each and keep the XCD 3-D form.  Samples in the first and in the
    last 64 pixels (the first finish workgroup and slot 65 535, geometry_cases._p4_edges), the rest at random: grad_value
    equals the oracle on every row a sample can touch, every other row is +0."""
    t = dict(inputs("P4", 4, "masked" if masked else "bilinear"))
    if not masked:
        t.pop("mask", None)
    pm, ac = gc.P4_MODE
    value = t["value"]
    if masked:
        value = torch.where(t["mask"][:, :, None, None] != 0, value, torch.full_like(value, float("nan")))
    from msda_triton_amd import multiscale_deformable_attention
    kw = dict(value_mask=t["mask"]) if masked else {}
    with options(**{**BASE, **gc.CASES["P4"]["options"]}):
        v = value.detach().requires_grad_(True)
        with counted({XCD3D: 1}, "P4 forward"):
            out = multiscale_deformable_attention(v, _shapes(t["levels"]), t["loc"], t["attn"], pm, ac, **kw)
        with counted({FLAT: 1, XCD3D: 3}, "P4 grad_value: count, place and gather 3-D, finish flat"):
            out.backward(t["grad_out"])
        info = launch_info()
    assert info["value_path"] == 2 and info["value_passes"] == 1, info
    gv = v.grad[0]  # [I, H, D]
    touched = lc.touched_rows(t["loc"], t["levels"], ac)[0]  # [I, H]
    if masked:
        touched &= (t["mask"][0] != 0)[:, None]
    assert not bool(gv.view(torch.int32)[~touched].any()), "a grad_value row that no sample touches is not +0"
    del touched
    for h, (nz, rows) in enumerate(_p4_reference()):
        want = torch.zeros(gv.shape[0], gv.shape[2], device=DEV)
        want[nz.to(DEV)] = rows.to(DEV)
        if masked:
            want[t["mask"][0] == 0] = 0
        assert int((want.abs().amax(dim=1) > 0)[:64].sum()) > 0 and int((want.abs().amax(dim=1) > 0)[-63:].sum()) > 0
        ne = (gv[:, h] != want).any(dim=1)
        assert not bool(ne.any()), f"P4 head {h}: {int(ne.sum())} grad_value rows differ from the oracle, first at pixel {int(ne.nonzero()[0])}"


# =========================================================================================================
# the forms the rest of the suite runs
# =========================================================================================================
def test_small_shapes_take_the_3d_and_2d_grids_never_the_flat_one():
    """Three SHAPE_MATRIX cases of tests/test_gpu_parity.py, forward and backward with the defaults: the XCD 3-D and the
    linear 2-D form are what small shapes get (so the rest of the suite covers those), the flat form is not."""
    from test_gpu_parity import SHAPE_MATRIX, rand_case, run_hip
    seen = {}
    for name, form in (("pairs_not_multiple_of_8", XCD3D), ("d32_vec_g8", XCD3D), ("one_query", LINEAR2D)):
        B, Q, H, D, levels, P = SHAPE_MATRIX[name]
        assert gc.expected_form(B * H, gc.gather_slots(Q, D), 1) == form
        c = rand_case(np.random.default_rng(7), B, Q, H, D, levels, P)
        before = launch_info()
        run_hip(c["value"], c["shapes"], c["loc"], c["attn"], c["grad_out"], "zeros", False)
        torch.cuda.synchronize()
        after = launch_info()
        moved = {k: after[k] - before[k] for k in gc.FORMS}
        assert moved[form] >= 1 and all(n == 0 for k, n in moved.items() if k != form), (name, moved)
        seen[form] = seen.get(form, 0) + moved[form]
    assert seen[XCD3D] >= 2 and seen[LINEAR2D] >= 1 and FLAT not in seen
