"""Cases, input builders and preconditions for tests/test_gpu_launch_geometry.py: launches whose (plane, slot) grid takes
the FLAT 1-D form of `plane_grid` (msda_triton_amd/csrc/msda_launch.hpp) — more than 65 535 planes in linear order, more
than 65 535 groups of eight planes in XCD order, or more than 65 535 slots.  A helper module, not a conftest.

Which form a launch takes ("Launch geometry"); `planes` = B * H, halved for two planes per workgroup:

    XCD 3-D     dim3(8, slots, ceil(planes / 8))   xcd_map on, slots <= 65535 and ceil(planes / 8) <= 65535
    linear 2-D  dim3(slots, planes)                xcd_map off, planes <= 65535
    flat 1-D    dim3(blocks)                       everything else: `decode_block` divides the block index

`xcd_map` is off when the option says so, and — decided inside plane_grid — when the planes cover the eight XCDs
unevenly (planes * 100 < ceil(planes / 8) * 8 * 85) or a skewed layout (128-byte rows 1 KB apart) has >= 320 slots.
`expected_form` below restates that rule from the text above, in Python integers.

Inputs are the dyadic numbers of tests/exact_cases.py, so every comparison with the fp64 oracle is an equality.  The
GPU file makes them on the device (large_cases.dev_*); `HostGen` makes the same distributions with numpy so that the
preconditions — bit budget, float32 oracle == float64 oracle, the arithmetic that reaches the form, the memory — are
held on the CPU (tests/test_geometry_cases.py).  The GPU file asserts float32 == float64 again on what it compares.

Slot counts that cannot reach the flat form inside the supported limits (B * H < 2^28, Q < 2^24, I < 2^22
for grad_value, S = L * P < 2^22, L <= 32), and so are left to the plane counts of P1 / P2:
  * count pass: slots = nsplit <= 64 (`sorted_ws_layout` caps the query slices per plane);
  * level-major place pass: slots = L * nsplit <= 32 * 64 = 2 048;
  * single-launch grad_value: slots = L * small_ns <= 32 * 4 = 128;
  * the LDS-served gathers: slots <= 2 * CUs (one or two 1024-thread workgroups per CU and plane);
  * gather-window pass: slots = ceil(win_cap / (256 / G)), win_cap = ceil(q_round * S / win).  The rounds over the queries
    hold planes * q_round * S * 16 bytes of records to 1.25 GiB, so a round has at most 83 886 080 / planes records per
    plane, in windows of 64 once there are that many.  With 4 windows per workgroup (G = 64, the fewest) slots > 65 535
    needs more than 16 776 960 records per plane and round, i.e. planes <= 5 — but under 7 planes the uneven-coverage rule
    (planes * 100 < 8 * 85) has switched to linear order, whose 2-D grid takes any slot count.  With planes >= 7:
    slots <= 83 886 080 / 7 / 64 / 4 = 46 812 < 65 535.  (Only the options "q_round" / "gather_win" could lift that; the
    defaults cannot.)  P3 keeps `value` frozen, so no grad_value pass runs at Q = 262 145.
The finish pass (slots = ceil(I / 64) <= 65 536 for I < 2^22) reaches the flat form with one slot to spare: P4.

Measured on an MI355X (tests/test_gpu_launch_geometry.py in a run of its own: 45 tests, 20 s; nothing asserts these),
slowest test and peak device memory per case: P1 3.1 s (the first discrete test builds the reference's module) / 0.14 GiB;
P2 1.3 s / 1.0 GiB; P1x2 0.4 s, P2x2 1.4 s / under 1.0 GiB; fused P1 / P2 0.2 s / 0.7 GiB; P3 0.03 s / 0.9 GiB (D = 33) and
3.6 GiB (D = 132); P4 2.8 s (seven oracle passes) / 3.1 GiB plain, 0.3 s / 3.9 GiB with the mask."""
import ctypes
import numpy as np
import torch

import exact_cases as ec

GiB = 1 << 30
MEMORY_LIMIT = 6 * GiB
GRID_LIMIT = 65535
F32_BITS = ec.F32_BITS
FORMS = ("grid_xcd3d_launches", "grid_linear2d_launches", "grid_flat_launches")
XCD3D, LINEAR2D, FLAT = FORMS

SMALL_LEVELS = [(2, 2), (1, 1)]
# name: dims, the options that select the form, the generator's bit counts and ranges
CASES = {
    # many planes, linear order
    "P1": dict(B=8200, H=8, Q=3, P=2, levels=SMALL_LEVELS, D=(4, 3), options=dict(xcd_map=0), padding_planes=False,
               gen=dict(loc_bits=7, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3)),
    # many planes, XCD order, the last group of eight has three padding blocks per slot
    "P2": dict(B=74899, H=7, Q=3, P=2, levels=SMALL_LEVELS, D=(4, 3), options={}, padding_planes=True,
               gen=dict(loc_bits=7, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3)),
    # the same with the plane count doubled: two planes per workgroup halve it (forward only)
    "P1x2": dict(B=16400, H=8, Q=3, P=2, levels=SMALL_LEVELS, D=(4,), options=dict(xcd_map=0), padding_planes=False,
                 planes_per_wg=2, gen=dict(loc_bits=7, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3)),
    "P2x2": dict(B=131075, H=8, Q=3, P=2, levels=SMALL_LEVELS, D=(4,), options={}, padding_planes=True, planes_per_wg=2,
                 gen=dict(loc_bits=7, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3)),
    # many slots: 65 536 * (256 / G) + 1 queries with G = 64 lanes per unit (D = 33 scalar, D = 132 in 16-byte pieces)
    "P3": dict(B=1, H=7, Q=65536 * 4 + 1, P=1, levels=[(4, 4)], D=(33, 132), options={}, padding_planes=True, G=64,
               gen=dict(loc_bits=6, attn_bits=2, vmax=3, gmax=3, lo=-0.3, hi=1.3)),
    # the finish pass with 65 536 slots of 64 pixels
    "P4": dict(B=1, H=7, Q=4096, P=2, levels=[(2047, 2049)], D=(4,), options=dict(value_path=2), padding_planes=True,
               gen=dict(loc_bits=8, attn_bits=1, vmax=1, gmax=1, lo=-0.1, hi=1.1)),
}
P4_EDGE_QUERIES = 64  # queries whose samples go to the first / to the last 64 pixels of the level
MODES = [("zeros", False), ("border", True)]  # (large_cases.MODES)
KINDS = ("bilinear", "ragged", "masked", "discrete", "fused")


def modes_for(name, kind="bilinear"):
    """P1 is small enough for both modes; the half-million planes of P2 take one per kind of input, alternating."""
    return MODES if name.startswith("P1") else [MODES[KINDS.index(kind) % 2]]


P4_MODE = ("border", False)  # y < 0 / y > 1 clamp to the first / last row; x * 2048 under align_corners would sit on pixels


def pixels(levels):
    return sum(h * w for h, w in levels)


def lane_group(D, vec):
    """Lanes per unit as the launchers pick them (pick_group): the power of two >= ceil(D / vec), between 4 and 64."""
    lanes = -(-D // vec)
    return min(64, max(4, 1 << (lanes - 1).bit_length()))


def vec_width(D):
    """Channels per lane in float32: 4 (16-byte pieces) when D is a multiple of 4, else the scalar path."""
    return 4 if D % 4 == 0 else 1


# ----------------------------------------------------------------------------------------- the grid form, restated
def expected_form(planes, slots, xcd_map, skewed=False):
    """The form plane_grid gives `planes` x `slots` workgroups, from the rule in this module's docstring."""
    groups = -(-planes // 8)
    if xcd_map and skewed and slots >= 320:
        xcd_map = 0
    if xcd_map and planes * 100 < groups * 8 * 85:
        xcd_map = 0
    if xcd_map and slots <= GRID_LIMIT and groups <= GRID_LIMIT:
        return XCD3D
    if not xcd_map and planes <= GRID_LIMIT:
        return LINEAR2D
    return FLAT


def gather_slots(Q, D):
    """Slots of the 256-thread forward / sample-gradient / discrete kernels: one query chunk of 256 / G units each."""
    return -(-Q // (256 // lane_group(D, vec_width(D))))


def finish_slots(I):  # noqa: E741
    """Slots of the finish pass with 4-lane groups (D = 4 in float32): 64 pixels each."""
    return -(-I // 64)


def form_arithmetic(name):
    """The inequalities that make `name` reach the flat form; returns {what: form} for its plane_grid launches."""
    c = CASES[name]
    planes = c["B"] * c["H"] // c.get("planes_per_wg", 1)
    xcd = c["options"].get("xcd_map", 1)
    I = pixels(c["levels"])  # noqa: E741
    assert c["B"] * c["H"] < 1 << 28 and c["Q"] < 1 << 24 and I < 1 << 22, "outside DESIGN.md §2"
    assert (planes % 8 != 0) == c["padding_planes"]
    forms = {}
    if name.startswith(("P1", "P2")):
        if xcd:
            assert -(-planes // 8) > GRID_LIMIT and planes * 100 >= -(-planes // 8) * 8 * 85
        else:
            assert planes > GRID_LIMIT
        for D in c["D"]:  # every pass of every route has a handful of slots: the plane count alone decides
            assert gather_slots(c["Q"], D) <= 4
            forms[f"gather D={D}"] = expected_form(planes, gather_slots(c["Q"], D), xcd)
        forms["grad_value passes"] = expected_form(planes, 32 * 64, xcd)  # (the most slots any of them can have)
    elif name == "P3":
        for D in c["D"]:
            assert lane_group(D, vec_width(D)) == c["G"]
            slots = gather_slots(c["Q"], D)
            assert slots == GRID_LIMIT + 2 and c["Q"] == (GRID_LIMIT + 1) * (256 // c["G"]) + 1
            assert D * 4 != 128, "a skewed layout would switch to linear order"
            forms[f"gather D={D}"] = expected_form(planes, slots, xcd)
            for half in (c["Q"] // 2, c["Q"] - c["Q"] // 2):  # the two query halves of the reference call
                assert expected_form(planes, gather_slots(half, D), xcd) == XCD3D
    elif name == "P4":
        assert I == 4194303 and I > GRID_LIMIT * 64 and finish_slots(I) == GRID_LIMIT + 1
        forms["finish"] = expected_form(planes, finish_slots(I), xcd)
        # count (<= 64 slices), level-major place (L * slices), gather windows (<= records / 16 / 64 + 1) and the forward
        for what, slots in (("count", 64), ("place", 64), ("gather", c["Q"] * c["P"] // 16 // 64 + 1),
                            ("forward", gather_slots(c["Q"], 4))):
            forms[what] = expected_form(planes, slots, xcd)
    return forms


def split_form(name, parts=2):
    """The form of the same call made on `parts` batch parts (P1 / P2): what the fused route is compared with."""
    c = CASES[name]
    planes = -(-c["B"] // parts) * c["H"]
    return expected_form(planes, 4, c["options"].get("xcd_map", 1))


# ----------------------------------------------------------------------------------------- generators
class HostGen:
    """numpy-backed: float32 CPU tensors of exact_cases' distributions."""
    device = "cpu"

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def grid(self, shape, vmax, bits, chunks=1):
        return torch.from_numpy(ec._grid(self.rng, shape, vmax, bits).astype(np.float32))

    def odd(self, shape, bits, lo, hi, chunks=1):
        return torch.from_numpy(ec._odd_multiples(self.rng, shape, bits, lo, hi).astype(np.float32))

    def weights(self, shape, bits, chunks=1):
        return torch.from_numpy((self.rng.integers(0, 2 ** bits + 1, size=shape) / 2 ** bits).astype(np.float32))

    def bernoulli(self, shape, keep):
        return torch.from_numpy((self.rng.random(shape) < keep).astype(np.uint8))


class DevGen:
    """The same on the device (large_cases.dev_*)."""

    def __init__(self, seed):
        import large_cases as lc
        self.lc, self.gen, self.device = lc, lc.generator(seed), lc.DEV

    def grid(self, shape, vmax, bits, chunks=1):
        return self.lc.dev_grid(shape, vmax, bits, self.gen, chunks=chunks)

    def odd(self, shape, bits, lo, hi, chunks=1):
        return self.lc.dev_odd_multiples(shape, bits, lo, hi, self.gen, chunks=chunks)

    def weights(self, shape, bits, chunks=1):
        return self.lc.dev_weights(shape, bits, self.gen, chunks=chunks)

    def bernoulli(self, shape, keep):
        return (torch.rand(shape, device=self.device, generator=self.gen) < keep).to(torch.uint8)


def seed_of(name, D, kind):
    import zlib
    return zlib.crc32(f"{name} {D} {kind}".encode())


def make_generator(name, D, kind, device):
    return (HostGen if device == "cpu" else DevGen)(seed_of(name, D, kind))


# ----------------------------------------------------------------------------------------- input builders
def bits_of(name, kind="bilinear"):
    g = CASES[name]["gen"]
    return dict(loc=g["loc_bits"], attn=g["attn_bits"], value=0, grad=0)


def build(name, D, kind, device):
    """The case's tensors on `device` ("cpu": numpy-made), float32.  `kind`:
      bilinear  value, loc [B, Q, H, L, P, 2], attn, grad_out
      ragged    per-level counts [2, 1]: loc [B, Q, H, 3, 2], attn [B, Q, H, 3], "counts"
      discrete  counts [P] * L in the ragged layout, "counts"
      masked    bilinear plus "mask" [B, I] uint8 (Bernoulli, 3 of 4 pixels real)
      fused     value, proj [B, Q, H, L, P, 3], ref [B, Q, 2], grad_out"""
    c, g = CASES[name], CASES[name]["gen"]
    # (the masked call: the bilinear inputs plus a mask from a generator of its own, so that references can be shared)
    gen = make_generator(name, D, "bilinear" if kind == "masked" else kind, device)
    B, H, Q, P, levels = c["B"], c["H"], c["Q"], c["P"], c["levels"]
    L, I = len(levels), pixels(levels)  # noqa: E741
    t = dict(levels=levels, value=gen.grid((B, I, H, D), g["vmax"], 0), grad_out=gen.grid((B, Q, H, D), g["gmax"], 0))
    if kind == "fused":
        proj = torch.empty(B, Q, H, L, P, 3, device=gen.device)
        proj[..., :2] = gen.odd((B, Q, H, L, P, 2), 4, -3.0, 3.0)
        proj[..., 2] = gen.grid((B, Q, H, L, P), 2, 0)
        t.update(proj=proj, ref=gen.weights((B, Q, 2), 3))
        return t
    if kind in ("ragged", "discrete"):
        counts = [2, 1][:L] if kind == "ragged" else [P] * L
        assert len(counts) == L
        pts = (sum(counts),)
        t["counts"] = counts
    else:
        pts = (L, P)
    t["loc"] = gen.odd((B, Q, H) + pts + (2,), g["loc_bits"], g["lo"], g["hi"])
    t["attn"] = gen.weights((B, Q, H) + pts, g["attn_bits"])
    if name == "P4":
        _p4_edges(t["loc"], g["loc_bits"], gen)
    if kind == "masked":
        t["mask"] = make_generator(name, D, "mask", device).bernoulli((B, I), 0.75)
    return t


def _p4_edges(loc, bits, gen):
    """P4: the first P4_EDGE_QUERIES queries sample the first 64 pixels of the level (row 0: y < 0 clamps to it under
    "border" padding, x * 2049 - 0.5 in (0, 64)), the next P4_EDGE_QUERIES the last 64 (the last row, x0 >= 1985)."""
    (h, w), n, scale = CASES["P4"]["levels"][0], P4_EDGE_QUERIES, 2 ** bits
    first = [k for k in range(1, scale, 2) if 0 < k * w / scale - 0.5 < 63]
    last = [k for k in range(1, scale + 16, 2) if k * w / scale - 0.5 > (w - 64) + 1]
    assert len(first) >= 4 and len(last) >= 4
    shape = loc[:, :n, ..., 0].shape

    def pick(ks):
        idx = (gen.weights(shape, 8) * 255).long() % len(ks)  # (any spread over the candidates will do)
        return torch.tensor(ks, dtype=torch.float32, device=loc.device)[idx] / scale

    loc[:, :n, ..., 0] = pick(first)
    loc[:, :n, ..., 1] = -pick(first)
    loc[:, n:2 * n, ..., 0] = pick(last)
    loc[:, n:2 * n, ..., 1] = 1 + pick(first)


def as_case(t, name, sel=None):
    """exact_cases' dict (numpy fp64, "bits") of the built tensors, or of the queries `sel` of batch element 0."""
    def np64(x):
        return x.detach().to("cpu", torch.float64).numpy()

    q = slice(None) if sel is None else torch.as_tensor(sel, device=t["grad_out"].device)
    b = slice(None) if sel is None else slice(0, 1)
    c = dict(value=np64(t["value"][b]), shapes=np.asarray(t["levels"], dtype=np.int64), loc=np64(t["loc"][b, q]),
             attn=np64(t["attn"][b, q]), grad_out=np64(t["grad_out"][b, q]), bits=bits_of(name))
    if "counts" in t:
        c["counts"] = list(t["counts"])
    return c


def apply_mask(c, mask):
    """The masked call's reference inputs: padding pixels hold zeros."""
    keep = mask.detach().cpu().numpy().astype(bool)
    return dict(c, value=np.where(keep[:, :, None, None], c["value"], 0.0))


# ----------------------------------------------------------------------------------------- P3: the compared queries
def p3_queries(D):
    """Queries a truncated or mis-decoded slot would move: the first and the last chunk, the chunks either side of slot
    65 535 / 65 536, and every 4 099th query."""
    c = CASES["P3"]
    Q, nu = c["Q"], 256 // lane_group(D, vec_width(D))
    chunks = [0, 1, GRID_LIMIT - 1, GRID_LIMIT, GRID_LIMIT + 1, (Q - 1) // nu]
    assert (Q - 1) // nu == GRID_LIMIT + 1 and max(chunks) * nu < Q
    qs = {q for ch in chunks for q in range(ch * nu, min(Q, (ch + 1) * nu))} | set(range(0, Q, 4099))
    return sorted(qs)


# ----------------------------------------------------------------------------------------- references
def oracle_all(c, pm, ac):
    """(fp64 oracle results, float32 oracle == float64 oracle bitwise) of a bilinear / ragged case dict."""
    r64 = ec._oracle_all(ec._oracle(), c, pm, ac, np.float64)
    r32 = ec._oracle_all(ec._oracle(), c, pm, ac, np.float32)
    return r64, all(np.array_equal(r32[k].astype(np.float64), r64[k]) for k in r64)


def discrete_all(c):
    """The same for a discrete case: test_discrete_sampling.ref_discrete in fp64, exact_cases' index form in float32."""
    r64 = ec._discrete_all(c, ec._ref_discrete, ec.F64)
    r32 = ec._discrete_all(c, ec._index_discrete, ec.F32)
    return r64, all(np.array_equal(r32[k].astype(np.float64), r64[k]) for k in r64)


def discrete_budget(c):
    absd = dict(c, value=np.abs(c["value"]), attn=np.abs(c["attn"]), grad_out=np.abs(c["grad_out"]))
    sums = ec._discrete_all(absd, ec._ref_discrete, ec.F64)
    b = c["bits"]
    frac = dict(out=b["attn"] + b["value"], grad_value=b["attn"] + b["grad"], grad_attn=b["value"] + b["grad"])
    return {k: frac[k] + ec._magnitude_bits(sums[k]) for k in frac}


def head_case(c, h):
    """Head `h` of a case as a problem of its own (heads are independent): keeps the host arrays of P4 small."""
    return dict(c, value=c["value"][:, :, h:h + 1], loc=c["loc"][:, :, h:h + 1], attn=c["attn"][:, :, h:h + 1],
                grad_out=c["grad_out"][:, :, h:h + 1])


# ----------------------------------------------------------------------------------------- memory
def _ws_bytes(family, B, I, H, D, Q, L, P, counts, flags=0):  # noqa: E741
    """The family's workspace query (host only, nothing is launched)."""
    from msda_triton_amd import _lib
    lib = _lib.load()
    if family == "plain":
        return int(lib.msda_bwd_workspace_bytes(B, I, H, D, Q, L, P, 4, 4, 0, flags))
    if family == "fused":
        return int(lib.msda_bwd_fused_workspace_bytes(B, I, H, D, Q, L, P, 4, 4, 0, 0))
    arr = (ctypes.c_int32 * L)(*counts)
    fn = lib.msda_bwd_ragged_workspace_bytes if family == "ragged" else lib.msda_bwd_discrete_workspace_bytes
    return int(fn(B, I, H, D, Q, L, ctypes.cast(arr, ctypes.c_void_p), 4, 4, 0, flags))


def device_bytes(name, D, kind, options=None):
    """Bytes of device memory a test of this case holds at once: inputs, results, the results of the reference call it
    is compared with on the device (P3: two query halves; fused: two batch halves and the unfused composition), the
    touched-row map of P4, and the family's workspace under `options` (set for the query, restored afterwards)."""
    from msda_triton_amd import _lib
    c = CASES[name]
    B, H, Q, P, levels = c["B"], c["H"], c["Q"], c["P"], c["levels"]
    L, I = len(levels), pixels(levels)  # noqa: E741
    counts = ([2, 1][:L] if kind == "ragged" else [P] * L) if kind in ("ragged", "discrete") else None
    S = sum(counts) if counts else L * P
    rows = (B * I * H * D + B * Q * H * D) * 4          # value, grad_out
    sampling = B * Q * H * S * 3 * 4 + (B * Q * 2 * 4 if kind == "fused" else 0)
    inputs = rows + sampling + (B * I if kind == "masked" else 0)
    results = rows + sampling                              # out, grad_value, grad_loc / grad_attn or grad_proj
    compared = results * (2 if kind == "fused" else 1) if name != "P4" else B * I * H * 9
    opts = dict(c["options"], **(options or {}))
    old = {k: _lib.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        family = {"ragged": "ragged", "discrete": "discrete", "fused": "fused"}.get(kind, "plain")
        ws = _ws_bytes(family, B, I, H, D, Q, L, P, counts)
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    return inputs + results + compared + ws, ws  # (ws == 0: the route needs none, e.g. the single-launch grad_value kernel)
