"""CPU: the preconditions of tests/geometry_cases.py, which tests/test_gpu_launch_geometry.py relies on — every case
reaches the grid form it is there for (the arithmetic, restated from the rule), is exact in float32 on what the GPU
file compares (bit budget <= 24, float32 oracle == float64 oracle), and fits 6 GiB of device memory (its tensors plus
the answer of its family's workspace query, a host-only call)."""
import numpy as np
import pytest

import exact_cases as ec
import geometry_cases as gc

P12 = ["P1", "P2"]
# the routes of the GPU file that need a workspace, and the options that select them
SORTED = dict(value_path=2)


def _case(name, D, kind="bilinear"):
    t = gc.build(name, D, kind, "cpu")
    return t, gc.as_case(t, name)


def _assert_exact(c, pm, ac, what, tensors=ec.TENSORS):
    ref, exact = gc.oracle_all(c, pm, ac)
    assert exact, f"{what}: the float32 and float64 oracles differ"
    bud = ec.budget(c, pm, ac)
    assert max(bud[k] for k in tensors) <= gc.F32_BITS, (what, bud)
    # no sample on an integer pixel coordinate, where grad_loc is discontinuous (an axis of one pixel under align_corners
    # is outside the rule: its coordinate is x * 0), exact_cases.precondition
    pix = ec.pixel_coordinates(c, ac)
    wh = np.stack([c["shapes"][:, 1], c["shapes"][:, 0]], -1).reshape(1, 1, 1, -1, 1, 2)
    assert not ((pix == np.round(pix)) & ~((wh == 1) & bool(ac))).any(), what
    return ref


# ----------------------------------------------------------------------------------------- the form each case reaches
def test_every_case_reaches_the_flat_form_by_arithmetic():
    for name in ("P1", "P2", "P1x2", "P2x2", "P3"):
        forms = gc.form_arithmetic(name)
        assert forms and set(forms.values()) == {gc.FLAT}, (name, forms)
    p4 = gc.form_arithmetic("P4")
    assert p4.pop("finish") == gc.FLAT and set(p4.values()) == {gc.XCD3D}, p4
    # the reference calls the fused route is compared with: two batch halves, each with a 3-D / 2-D grid
    assert gc.split_form("P1") == gc.LINEAR2D and gc.split_form("P2") == gc.XCD3D


def test_the_case_table_says_what_the_issue_says():
    c = gc.CASES
    assert (c["P1"]["B"] * c["P1"]["H"], c["P2"]["B"] * c["P2"]["H"]) == (65600, 524293)
    assert -(-524293 // 8) == 65537 and 524293 % 8 == 5
    assert (c["P1x2"]["B"] * 8 // 2, c["P2x2"]["B"] * 8 // 2) == (65600, 524300) and -(-524300 // 8) > 65535
    assert c["P3"]["Q"] == 262145 and gc.gather_slots(262145, 33) == gc.gather_slots(262145, 132) == 65537
    assert gc.pixels(c["P4"]["levels"]) == 4194303 and gc.finish_slots(4194303) == 65536
    assert gc.lane_group(33, 1) == gc.lane_group(132, 4) == 64 and gc.lane_group(4, 4) == gc.lane_group(3, 1) == 4


def test_expected_form_on_small_shapes():
    """The three SHAPE_MATRIX cases the GPU file uses to show the forms the rest of the suite runs."""
    assert gc.expected_form(15, 6, 1) == gc.XCD3D       # pairs_not_multiple_of_8: 3 * 5 planes
    assert gc.expected_form(16, 9, 1) == gc.XCD3D       # d32_vec_g8
    assert gc.expected_form(1, 1, 1) == gc.LINEAR2D     # one_query: one plane covers the XCDs unevenly
    assert gc.expected_form(7, 65537, 1) == gc.FLAT and gc.expected_form(6, 65537, 1) == gc.LINEAR2D
    assert gc.expected_form(65535, 1, 0) == gc.LINEAR2D and gc.expected_form(65536, 1, 0) == gc.FLAT
    assert gc.expected_form(65535 * 8, 1, 1) == gc.XCD3D and gc.expected_form(65535 * 8 + 1, 1, 1) == gc.FLAT


# ----------------------------------------------------------------------------------------- exactness
@pytest.mark.parametrize("D", [4, 3])
@pytest.mark.parametrize("name", P12)
def test_many_planes_are_exact_in_float32(name, D):
    """Whole tensors in the modes the GPU file runs (geometry_cases.modes_for): the uniform, the per-level-count and the
    masked inputs."""
    for kind in ("bilinear", "ragged", "masked"):
        t, c = _case(name, D, kind)
        if kind == "masked":
            c = gc.apply_mask(c, t["mask"])
        for pm, ac in gc.modes_for(name, kind):
            _assert_exact(c, pm, ac, f"{name} D={D} {kind} {pm} {ac}")


@pytest.mark.parametrize("name", P12 + ["P3"])
def test_discrete_inputs_are_exact_in_float32(name):
    for D in gc.CASES[name]["D"]:
        t = gc.build(name, D, "discrete", "cpu")
        c = gc.as_case(t, name, gc.p3_queries(D) if name == "P3" else None)
        ref, exact = gc.discrete_all(c)
        assert exact, (name, D)
        assert max(gc.discrete_budget(c).values()) <= gc.F32_BITS


@pytest.mark.parametrize("name", ["P1x2", "P2x2"])
def test_two_planes_per_workgroup_inputs_are_exact_in_float32(name):
    _, c = _case(name, 4)
    for pm, ac in gc.modes_for(name):
        _assert_exact(c, pm, ac, f"{name} {pm} {ac}", tensors=("out",))


@pytest.mark.parametrize("D", [33, 132])
def test_many_slots_are_exact_on_the_compared_queries(D):
    qs = gc.p3_queries(D)
    nu = 256 // 64
    assert {0, nu - 1, 65535 * nu - 1, 65535 * nu, 65536 * nu - 1, 65536 * nu, 4099, 4099 * 63} <= set(qs)
    assert qs[-1] == gc.CASES["P3"]["Q"] - 1 and len(qs) < 100
    c = gc.as_case(gc.build("P3", D, "bilinear", "cpu"), "P3", qs)
    for pm, ac in gc.MODES:
        _assert_exact(c, pm, ac, f"P3 D={D} {pm} {ac}", tensors=("out", "grad_loc", "grad_attn"))


def test_finish_pass_case_is_exact_and_reaches_both_ends():
    t, c = _case("P4", 4)
    (h, w), n = gc.CASES["P4"]["levels"][0], gc.P4_EDGE_QUERIES
    pm, ac = gc.P4_MODE
    pix = ec.pixel_coordinates(c, ac)  # [1, Q, H, 1, P, 2]: (x, y)
    x0, y = np.floor(pix[..., 0]), pix[..., 1]
    assert (y[:, :n] < 0).all() and (x0[:, :n] >= 0).all() and (x0[:, :n] < 63).all()          # pixels 0 .. 63
    assert (y[:, n:2 * n] > h - 1).all() and (x0[:, n:2 * n] >= w - 64).all()                   # the last 64 pixels
    I = gc.pixels(gc.CASES["P4"]["levels"])  # noqa: E741
    for head in range(gc.CASES["P4"]["H"]):
        ch = gc.head_case(c, head)
        ref = _assert_exact(ch, pm, ac, f"P4 head {head}", tensors=("grad_value",))
        gv = ref["grad_value"].reshape(I, -1)
        assert np.abs(gv[:64]).max() > 0 and np.abs(gv[I - 63:]).max() > 0, "an end of the level got no gradient"
        assert np.abs(gv[64:I - 63]).max() > 0


# ----------------------------------------------------------------------------------------- memory
ROUTES = [("bilinear", {}), ("bilinear", SORTED), ("bilinear", dict(value_path=2, place_path=1)), ("masked", SORTED),
          ("ragged", {}), ("ragged", SORTED), ("discrete", {}), ("discrete", SORTED), ("fused", {}), ("fused", SORTED)]


@pytest.mark.parametrize("name", list(gc.CASES))
def test_every_case_fits_six_gib(name):
    case = gc.CASES[name]
    for D in case["D"]:
        for kind, opts in ROUTES:
            if name == "P4" and (kind not in ("bilinear", "masked") or not opts):
                continue
            need, ws = gc.device_bytes(name, D, kind, opts)
            assert need < gc.MEMORY_LIMIT, (name, D, kind, opts, need)
            if opts.get("value_path") == 2:
                assert ws > 0, f"{name} D={D} {kind}: the workspace query refuses the shape"
    if name == "P4":
        need, ws = gc.device_bytes("P4", 4, "bilinear", SORTED)
        assert 3 * gc.GiB < need < 4 * gc.GiB and ws > 2 * gc.GiB, (need, ws)  # scratch rows and cell tables of 7 planes
