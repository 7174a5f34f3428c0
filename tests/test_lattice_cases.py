"""The lattice fixtures of tests/exact_cases.py (kind "lattice") on the CPU: sampling points ON integer pixel
coordinates, where grad_loc is discontinuous, "border" switches its gradient off (px <= 0, px >= n - 1) and "zeros"
drops corners (px = -1, n - 1, n).  The behaviour there is fully defined — three independent statements of the operator
(the C oracle, grid_sample with autograd, the gather formulation) agree bit for bit in all four tensors — so
tests/test_gpu_lattice.py can hold the kernels to EQUALITY with nothing masked.  Here: the precondition, that agreement,
a tally showing that every class of position (and every joint class of a corner) is among the inputs, and emulated wrong
kernels that differ from the reference on these fixtures and on none of the off-lattice ones."""
import numpy as np
import pytest
import torch

import exact_cases as ec
from exact_cases import MODES, TENSORS

RUN_IDS = [f"{n}-{pm}_{int(ac)}" for n, pm, ac in ec.LATTICE_RUNS]
FULL = [n for n in ec.LATTICE if ec.CASES[n][2]["align"] is not None]
UNIVERSAL = [n for n in ec.LATTICE if ec.CASES[n][2]["align"] is None]
OFF_LATTICE = ["d8_vec_g4", "d5_scalar", "many_levels", "ragged_363"]  # existing cases: no sample on the lattice


def _t(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad)


# ----------------------------------------------------------------------------------------- the precondition
@pytest.mark.parametrize("name,pm,ac", ec.LATTICE_RUNS, ids=RUN_IDS)
def test_precondition_holds(name, pm, ac):
    bud = ec.precondition(name, pm, ac)
    share = ec.lattice_share(ec.get_case(name), ac)
    print(f"{name} {pm} {ac}: budget {bud}, {share:.1%} of the samples have a coordinate on an integer")
    assert set(bud) == set(TENSORS) and max(bud.values()) <= 24 and share >= 0.5


def test_a_full_lattice_is_off_the_lattice_in_the_other_align_mode():
    """The share is not vacuous, and the precondition refuses a mode the case was not made for."""
    for name in FULL:
        align = ec.CASES[name][2]["align"]
        assert ec.lattice_share(ec.get_case(name), not align) < ec.lattice_share(ec.get_case(name), align)
        with pytest.raises(AssertionError):
            ec.precondition(name, "zeros", not align)


def test_the_issues_shares():
    """75 % and 82 % of the samples of the two smallest full lattices have a coordinate on an integer (one point per level)."""
    shares = {al: ec.lattice_share(ec.get_case(f"lat_{tag}_d4"), al) for tag, al in (("f", False), ("t", True))}
    print(shares)
    assert shares[False] >= 0.7 and shares[True] >= 0.8


def test_generator_properties():
    for name in FULL:
        kind, (B, Q, H, D, levels, P), kw, _ = ec.CASES[name]
        c, al = ec.get_case(name), kw["align"]
        assert levels == ec.LATTICE_LEVELS[al] and (B, H) == (2, 2)
        pix = ec.pixel_coordinates(c, al)
        for lvl, (h, w) in enumerate(levels):  # every (x, y) pair of -2, -1.5, ..., n + 1.5 per level
            p = pix[:, :, :, lvl, :(c["counts"][lvl] if "counts" in c else None)].reshape(-1, 2)
            assert np.array_equal(p * 2, np.round(p * 2))  # halves, exactly
            xs = [0.0] if (al and w == 1) else list(np.arange(-4, 2 * w + 4) / 2)
            ys = [0.0] if (al and h == 1) else list(np.arange(-4, 2 * h + 4) / 2)
            assert {(x, y) for x, y in p.tolist()} == {(x, y) for x in xs for y in ys}, (name, lvl)
    for name in UNIVERSAL:
        c = ec.get_case(name)
        vals, share = np.unique(c["loc"], return_counts=True)
        assert set(vals) == {v for v, _ in ec.UNIVERSAL_VALUES} | set(ec.UNIVERSAL_NEIGHBOURS)
        on = np.isin(c["loc"], [v for v, _ in ec.UNIVERSAL_VALUES])
        assert 0.75 < on.mean() < 0.95 and np.signbit(c["loc"][c["loc"] == 0]).any()  # -0.0 is there
    assert ec.get_case("lat_f_c")["counts"] == [2, 5, 1, 3] and ec.get_case("lat_u_c")["loc"].shape == (2, 200, 2, 10, 2)


# ----------------------------------------------------------------------------------------- three references, bit for bit
def _torch_all(fn, c, pm, ac):
    d = ec.dense(c)
    v, l, a = _t(d["value"], True), _t(d["loc"], True), _t(d["attn"], True)
    out = fn(v, _t(d["shapes"]), l, a, pm, ac)
    out.backward(_t(d["grad_out"]))
    gl, ga = l.grad.numpy(), a.grad.numpy()
    if "counts" in c:
        gl, ga = ec._unpad(gl, c["counts"]), ec._unpad(ga, c["counts"])
    return dict(out=out.detach().numpy(), grad_value=v.grad.numpy(), grad_loc=gl, grad_attn=ga)


@pytest.mark.parametrize("name,pm,ac", ec.LATTICE_RUNS, ids=RUN_IDS)
def test_three_references_agree_bit_for_bit(name, pm, ac):
    """The C oracle (float64; the precondition holds its float32 build to it), F.grid_sample with autograd and the gather
    formulation: out, grad_value, grad_loc and grad_attn equal, every sample compared."""
    from msda_triton_amd.functional import _gather_multiscale_deformable_attention, native_multiscale_deformable_attention
    c, ref = ec.get_case(name), ec.checked_reference(name, pm, ac)
    for fn in (native_multiscale_deformable_attention, _gather_multiscale_deformable_attention):
        got = _torch_all(fn, c, pm, ac)
        for k in TENSORS:
            assert got[k].dtype == np.float64 and np.array_equal(got[k], ref[k]), (name, pm, ac, fn.__name__, k)
    assert np.array_equal(ec.real_grad_loc(c, ec.location_gradients(c, pm, ac)), ref["grad_loc"])  # the mutants' base


# ----------------------------------------------------------------------------------------- coverage tally
def _tally(name, ac):
    """-> per level (classes of x [10, n], classes of y [10, n]) of the case's real samples."""
    c = ec.get_case(name)
    pix = ec.pixel_coordinates(c, ac)
    out = []
    for lvl, (h, w) in enumerate(c["shapes"].tolist()):
        p = pix[:, :, :, lvl, :(c["counts"][lvl] if "counts" in c else None)].reshape(-1, 2)
        out.append((ec.position_classes(p[:, 0], w), ec.position_classes(p[:, 1], h)))
    return out


def _possible(n):
    """The classes an axis of n pixels has: no interior integer below three pixels, no interior at all on one."""
    return [i for i, k in enumerate(ec.POSITION_CLASSES)
            if not (k == "interior integer" and n < 3) and not (k == "interior half" and n < 2)]


@pytest.mark.parametrize("name", FULL)
def test_every_class_of_position_is_present(name):
    """Per level and axis every class the axis has, jointly: each pair (class of x, class of y) occurs — the corners of
    corners, (-1, -1), (w - 1, h - 1), (w, h), among them.  Level 0 has all ten classes on both axes: 100 joint classes."""
    al = ec.CASES[name][2]["align"]
    c = ec.get_case(name)
    for lvl, ((h, w), (cx, cy)) in enumerate(zip(c["shapes"].tolist(), _tally(name, al))):
        if al and (w == 1 or h == 1):  # the coordinate of a one-pixel axis is x * 0: always 0 = n - 1
            assert w > 1 or (cx[3].all() and cx[6].all())
            assert h > 1 or (cy[3].all() and cy[6].all())
        joint = cx[:, None, :] & cy[None, :, :]
        seen = joint.any(-1)
        for i in ([3] if (al and w == 1) else _possible(w)):
            for j in ([3] if (al and h == 1) else _possible(h)):
                assert seen[i, j], (name, lvl, ec.POSITION_CLASSES[i], ec.POSITION_CLASSES[j])
        print(f"{name} level {lvl} ({h} x {w}): {int(seen.sum())} joint classes, per class of x:",
              dict(zip(ec.POSITION_CLASSES, cx.sum(-1).tolist())))
    cx, cy = _tally(name, al)[0]
    assert (cx[:, None, :] & cy[None, :, :]).any(-1).all()  # 10 x 10 at level 0


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("name", UNIVERSAL)
def test_universal_values_land_on_the_kinks_of_arbitrary_sizes(name, ac):
    """align_corners: px = 0 and px = n - 1 on every axis (the border-clip kinks), interior integers on the odd axes;
    otherwise interior integers on the odd axes and both half-pixel margins."""
    c = ec.get_case(name)
    for (h, w), (cx, cy) in zip(c["shapes"].tolist(), _tally(name, ac)):
        for n, cls in ((w, cx), (h, cy)):
            have = {k for k, row in zip(ec.POSITION_CLASSES, cls) if row.any()}
            want = {"px = 0", "px = n - 1"} if ac else {"-1 < px < 0", "n - 1 < px < n"}
            if n % 2 and n >= 3:
                want.add("interior integer")
            assert want <= have, (name, ac, n, have)


# ----------------------------------------------------------------------------------------- emulated wrong kernels
def _mutant_modes(rule, name):
    return [(pm, ac) for pm, ac in ec.lattice_modes(name) if ec.LATTICE_MUTANTS[rule] in (None, pm)]


# what the universal values can show: x = 0.5 is an interior integer of the odd axes in every mode; px = 0 and px = n - 1
# need align_corners; px = -1 is no universal value
UNIVERSAL_SHOWS = {"left_cell_at_integers": MODES, "border_gradient_alive_at_zero": [("border", True)],
                   "border_gradient_after_clamp": [("border", True)], "zeros_drops_minus_one": []}


@pytest.mark.parametrize("rule", list(ec.LATTICE_MUTANTS))
def test_mutants_differ_on_the_lattice_only(rule):
    for name in ec.LATTICE:
        c = ec.get_case(name)
        modes = _mutant_modes(rule, name) if name in FULL else UNIVERSAL_SHOWS[rule]
        for pm, ac in modes:
            want = ec.checked_reference(name, pm, ac)["grad_loc"]
            got = ec.real_grad_loc(c, ec.location_gradients(c, pm, ac, rule))
            off = got != want
            assert off.any(), (rule, name, pm, ac)
            pix = ec.pixel_coordinates(c, ac)
            on_grid = ec.real_samples(c, (pix == np.round(pix)).any(-1))
            assert on_grid[off.reshape(-1, 2).any(-1)].all()  # ... and only at samples on the lattice
            for dt in (ec.F32,) + tuple(ec.storage_types(name)):  # caught in every storage type
                assert not torch.equal(_t(got).float().to(dt), ec.expected(want, dt)), (rule, name, pm, ac, dt)
    for name in OFF_LATTICE:
        c = ec.get_case(name)
        for pm, ac in MODES:
            got = ec.real_grad_loc(c, ec.location_gradients(c, pm, ac, rule))
            assert np.array_equal(got, ec.reference(name, pm, ac)["grad_loc"]), (rule, name, pm, ac)


# ----------------------------------------------------------------------------------------- the fused families' draws
import head_dim_cases as hd  # noqa: E402

FUSED = [(f, rd, ac, u) for u in (False, True) for f in hd.FUSED_FAMILIES for rd in hd.fused_ref_dims(f) for ac in (False, True)]
FUSED_IDS = [f"{f}-ref{rd}-ac{int(ac)}{'-universal' if u else ''}" for f, rd, ac, u in FUSED]
FULL_FUSED = [c for c in FUSED if not c[3]]


@pytest.mark.parametrize("storage", list(hd.FUSED_STORAGE))
@pytest.mark.parametrize("family,ref_dim,ac,universal", FUSED, ids=FUSED_IDS)
def test_fused_prologues_form_the_lattice_points_exactly(family, ref_dim, ac, universal, storage):
    """The family's prologue in float32 — as PyTorch states it, as `offset * factor` and as `offset / (1 / factor)` —
    gives the float64 points bit for bit, from inputs that are what they were before they went into their storage types."""
    inp = hd.fused_lattice_inputs(family, storage, 32, ref_dim, ac, universal)
    want = inp["points"]
    p64, _ = hd.fused_sampling_inputs(family, inp["proj"].double(), inp["shapes"], inp["ref"].double(), inp["counts"])
    p32, _ = hd.fused_sampling_inputs(family, inp["proj"].float(), inp["shapes"], inp["ref"].float(), inp["counts"])
    assert p32.dtype == torch.float32 and np.array_equal(p64.numpy(), want) and np.array_equal(p32.double().numpy(), want)
    off, factor = inp["proj"][..., :2].float(), _t(inp["factor"]).float()
    assert inp["zero_offsets"] == (not off.any()) == ((universal or bool(ac)) and ref_dim == 2)
    if not inp["zero_offsets"]:  # every factor a power of two: its float32 reciprocal is exact as well
        m, _ = np.frexp(inp["factor"])
        assert (m == 0.5).all()
    base = _t(want).float() - off * factor  # the reference point of each sample, broadcast (exact: all dyadic)
    for pts in (base + off * factor, base + off / (1.0 / factor), torch.addcmul(base, off, factor)):
        assert pts.dtype == torch.float32 and np.array_equal(pts.double().numpy(), want)
    for k, dt in zip(("value", "proj", "ref"), hd.FUSED_STORAGE[storage]):
        assert inp[k].dtype == getattr(torch, dt)
    f32 = hd.fused_lattice_inputs(family, "f32", 32, ref_dim, ac, universal)  # the same draw in float32: nothing moved in 16 bits
    assert torch.equal(inp["proj"][..., :2].double(), f32["proj"][..., :2].double()) and torch.equal(inp["ref"].double(), f32["ref"].double())


@pytest.mark.parametrize("family,ref_dim,ac,universal", FULL_FUSED, ids=FUSED_IDS[:len(FULL_FUSED)])
def test_fused_draws_land_on_every_class_of_position(family, ref_dim, ac, universal):
    """Level 0 (both axes have all ten classes): each class on each axis, and the corners of corners (-1, -1),
    (w - 1, h - 1), (w, h); at least half of the samples have a coordinate on an integer."""
    inp = hd.fused_lattice_inputs(family, "f32", 32, ref_dim, ac)
    levels, pts = inp["shapes"].tolist(), inp["points"]
    h, w = levels[0]
    p0 = (pts[:, :, :, :inp["counts"][0]] if inp["counts"] else pts[:, :, :, 0]).reshape(-1, 2)
    px = p0 * (np.asarray([w, h]) - 1) if ac else p0 * np.asarray([w, h]) - 0.5
    cx, cy = ec.position_classes(px[:, 0], w), ec.position_classes(px[:, 1], h)
    assert cx.any(-1).all() and cy.any(-1).all(), (cx.sum(-1), cy.sum(-1))
    for i in (1, 6, 8):  # px = -1, n - 1, n on both axes at once
        assert (cx[i] & cy[i]).any(), ec.POSITION_CLASSES[i]
    c = hd._as_case(inp, _t(pts), _t(pts[..., 0]), inp["value"].double())
    share = ec.lattice_share(c, ac)
    print(family, ref_dim, ac, f"{share:.1%} of the samples have a coordinate on an integer")
    assert share >= 0.5


@pytest.mark.parametrize("family,ref_dim,ac,universal", FUSED[len(FULL_FUSED):], ids=FUSED_IDS[len(FULL_FUSED):])
def test_universal_fused_draws_land_on_the_kinks(family, ref_dim, ac, universal):
    """As the plain universal cases: px = 0 and px = n - 1 on every axis under align_corners, the half-pixel margins
    otherwise, interior integers on the odd axes in both."""
    inp = hd.fused_lattice_inputs(family, "f32", 32, ref_dim, ac, universal)
    pts = inp["points"]
    s0 = 0
    for lvl, (h, w) in enumerate(inp["shapes"].tolist()):
        n = inp["counts"][lvl] if inp["counts"] else None
        p = (pts[:, :, :, s0:s0 + n] if n else pts[:, :, :, lvl]).reshape(-1, 2)
        s0 += n or 0
        for axis, size in ((0, w), (1, h)):
            px = p[:, axis] * (size - 1) if ac else p[:, axis] * size - 0.5
            have = {k for k, row in zip(ec.POSITION_CLASSES, ec.position_classes(px, size)) if row.any()}
            want = {"px = 0", "px = n - 1"} if ac else {"-1 < px < 0", "n - 1 < px < n"}
            if size % 2 and size >= 3:
                want.add("interior integer")
            assert want <= have, (family, ref_dim, ac, lvl, size, have)


@pytest.mark.parametrize("D", [5, 32])
@pytest.mark.parametrize("family,ref_dim,ac,universal", FUSED, ids=FUSED_IDS)
def test_the_reference_alone_stays_within_the_float32_bounds(family, ref_dim, ac, universal, D):
    """The float32 host composition against the float64 one, no sample masked: the same points, so what is left is
    rounding — well inside FWD_TOL / BWD_TOL, the bounds tests/test_gpu_lattice.py holds the float32 kernels to."""
    from test_gpu_parity import BWD_TOL, FWD_TOL
    inp = hd.fused_lattice_inputs(family, "f32", D, ref_dim, ac, universal)
    for pm in ("zeros", "border"):
        want = hd.fused_reference(inp, pm, ac)
        got = hd.fused_reference(inp, pm, ac, real="float32")
        tols = [FWD_TOL[torch.float32]] + [BWD_TOL[torch.float32]] * 3
        for name, g, w, t in zip(("out", "grad_value", "grad_proj", "grad_ref"), got, want, tols):
            assert g.dtype == torch.float32
            torch.testing.assert_close(g, w.float(), msg=lambda m: f"{family} {ref_dim} {pm} {ac} {name}: {m}", **t)
