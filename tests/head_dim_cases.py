"""Which template instantiation a head dimension D reaches, restated from msda_launch.hpp (dispatch_gather,
dispatch_group, pick_group) so that the GPU tests can hold `msda_last_launch_info` to it.  A helper module, not a conftest.

  VEC     channels per lane: 16 bytes of the ARITHMETIC type (mixed storage computes in float32: 4), or 1 when D is no
          multiple of that or a row pointer is not 16-byte aligned;
  G       lanes per (b, q, h) unit: pick_group(ceil(D / VEC)), one of 4, 8, 16, 32, 64;
  chunks  ceil(D / (G * VEC)) trips of the kernels' channel loop.

These are different code, not different sizes: group_sum / group_max stay inside a DPP row up to G = 16 and cross rows at
32 and 64; the sample-gradient kernel has a reduce-scatter body (G 4, 8), a one-chunk body (G 16-64) and a chunked loop;
the fused forward repeats its prologue per chunk; a group or last chunk that D does not fill runs the tail guards.

The cases themselves (inputs on which the operator is exact) live in tests/exact_cases.py: "hd<D>_p3", "hd<D>_c25",
"hd<D>_disc" on the base shape B = 2, Q = 11, H = 2, levels [(5, 4), (3, 2)]."""
import functools

import exact_cases as ec

HEAD_DIMS = ec.HEAD_DIMS
STORAGES = ("f32", "f64", "fp16", "bf16", "f32_vbf16", "f32_vf16")
# bytes of the type the kernels compute and sample in (T of run_fwd<T, TV>): it alone sets VEC, also for 16-bit value rows
ARITH_BYTES = {"f32": 4, "f64": 8, "fp16": 2, "bf16": 2, "f32_vbf16": 4, "f32_vf16": 4}
SIXTEEN_BIT = ("fp16", "bf16")
WAVE = 64


def pick_group(lanes_needed):
    for g in (4, 8, 16, 32):
        if lanes_needed <= g:
            return g
    return 64


def instantiation(storage, D, aligned=True):
    """(VEC, G, chunks) of a call with head dimension D; aligned=False: a row pointer is not 16-byte aligned."""
    vec = 16 // ARITH_BYTES[storage]
    if not aligned or D % vec:
        vec = 1
    g = pick_group(-(-D // vec))
    return vec, g, -(-D // (g * vec))


def partly_filled(storage, D, aligned=True):
    """The last chunk's lanes are not all in use, or its last lane's channels are not (never, as VEC divides D)."""
    vec, g, _ = instantiation(storage, D, aligned)
    return -(-D // vec) % g != 0


def classes(storage, dims=HEAD_DIMS):
    """The classes a list of head dimensions reaches: (path, "g<G>"), (path, "chunks2+"), (path, "partial")."""
    got = set()
    for D in dims:
        vec, g, chunks = instantiation(storage, D)
        path = "vec" if vec > 1 else "scalar"
        got.add((path, f"g{g}"))
        if chunks >= 2:
            got.add((path, "chunks2+"))
        if chunks >= 3:
            got.add((path, "chunks3+"))
        if partly_filled(storage, D):
            got.add((path, "partial"))
    return got


def required(storage):
    need = {(p, c) for p in ("vec", "scalar") for c in ("g32", "g64", "chunks2+", "partial")}
    if storage in SIXTEEN_BIT:
        need.add(("vec", "g16"))  # 16-bit rows reach 8 lanes at D = 64: G = 16 is new there too
    return need


def expect_info(storage, D, aligned=True, value_aligned=True):
    """The nine launch-info keys of a forward + backward.  `aligned`: value / out / grad_out rows as the forward and the
    sample gradients see them; grad_value's kernels look at grad_out and grad_value only (value_aligned)."""
    f = instantiation(storage, D, aligned)
    v = instantiation(storage, D, value_aligned)
    keys = {}
    for fam, inst in (("fwd", f), ("sample", f), ("value", v)):
        keys.update({f"{fam}_vec": inst[0], f"{fam}_group": inst[1], f"{fam}_chunks": inst[2]})
    return keys


def assert_info(info, want, what, families=("fwd", "sample", "value")):
    got = {k: info[k] for k in want if k.split("_")[0] in families}
    assert got == {k: v for k, v in want.items() if k in got}, (what, got, want)


# ----------------------------------------------------------------------------------------- forced variants
# one-wave-per-unit forward (option unit_fwd = 2; launch_gather): 16-byte pieces of a 4-byte-accumulating operator, D / VEC a
# power of two up to 64.  (storage, D): the fwd_variant the option gives and, where it is 2, fwd_group = D / VEC
UNIT_FWD = {
    ("f32", 128): 2, ("f32", 256): 2,       # D / 4 = 32, 64
    ("bf16", 256): 2,                        # D / 8 = 32
    ("f32", 68): 0, ("f32", 132): 0,         # 17, 33 lanes: no power of two — declined, the 256-thread kernel
    ("bf16", 136): 0, ("bf16", 264): 0,      # 17, 33 lanes
    ("f64", 128): 0,                         # float64 accumulators: the variant does not exist
}
# LDS-served coarse levels (option lds_levels = 2; launch_gather): the forward exists for VEC = 4 and G <= 16, the sample
# gradients for G of 4 and 8 — so at G = 32 and G = 64 the option is DECLINED and both take the 256-thread kernels
LDS_LEVELS = {("f32", 68): (0, 0), ("f32", 132): (0, 0), ("f32_vbf16", 68): (0, 0), ("f32_vbf16", 132): (0, 0)}


def case_name(D, kind):
    return f"hd{D}_{kind}"


# ----------------------------------------------------------------------------------------- the fused module-core families
# On random inputs (as tests/test_gpu_fused_ragged.make draws them: randn value, projection randn * 1.5, reference points
# in [0, 1)), against the family's prologue in PyTorch float64 on the host around the C oracle (fused_reference).
FUSED_FAMILIES = ("uniform", "ragged", "levelref", "levelref_masked", "hfbox")
FUSED_NAMES = {"uniform": ["msda_fwd_fused", "msda_bwd_fused"], "ragged": ["msda_fwd_fused_ragged", "msda_bwd_fused_ragged"],
               "levelref": ["msda_fwd_fused_levelref", "msda_bwd_fused_levelref"],
               "levelref_masked": ["msda_fwd_fused_levelref", "msda_bwd_fused_levelref"],
               "hfbox": ["msda_fwd_fused_hfbox", "msda_bwd_fused_hfbox"]}
# name: (value, projection / result, reference points) as torch dtype names; the arithmetic type is float32 whenever the
# reference points are (the "s" variants: 16-bit value and projection; the "v" variants: 16-bit value only)
FUSED_STORAGE = {
    "f32": ("float32",) * 3, "f64": ("float64",) * 3, "bf16": ("bfloat16",) * 3, "fp16": ("float16",) * 3,
    "sbf16": ("bfloat16", "bfloat16", "float32"), "sf16": ("float16", "float16", "float32"),
    "vbf16": ("bfloat16", "float32", "float32"), "vf16": ("float16", "float32", "float32"),
}
FUSED_ARITH = {"f32": "f32", "f64": "f64", "bf16": "bf16", "fp16": "fp16", "sbf16": "f32", "sf16": "f32", "vbf16": "f32", "vf16": "f32"}
# one D per class of the table (16-byte path: G32, G64, two chunks, three chunks; scalar path: G32, G64, two chunks; and G16
# for 16-bit arithmetic); the 16-bit value variants of float32 arithmetic take the float32 classes at one D each
FUSED_DIMS = {
    "f32": (68, 132, 260, 520, 17, 33, 65), "f64": (34, 66, 130, 260, 17, 33, 65),
    "bf16": (72, 136, 264, 520, 17, 33, 65, 130), "fp16": (72, 136, 264, 520, 17, 33, 65, 130),
    "sbf16": (68, 132, 260, 33), "sf16": (68, 132, 260, 33), "vbf16": (68, 132, 260, 33), "vf16": (68, 132, 260, 33),
}
FUSED_AGAINST_FP64 = ("f32", "f64")  # the others: against the float32 kernels on the same rounded inputs
FUSED_MODES = (("zeros", False), ("border", True))
FUSED_SMALL, FUSED_LARGE = 6, 70  # samples per unit: P = 3 or counts [2, 4]; P = 35 or counts [30, 40] — more than 64 lanes
KINK_CAP = 0.02                   # share of offset gradients compared away from grid kinks, at most (the digest test's cap)


def fused_lp_limit(D, elem_size):
    """msda_fused_lp_limit restated: the samples of a unit the fused kernels hold in one LDS pass — 48 KiB of records of
    16 + 7 accumulators bytes for the 256 / G units of a workgroup, less one — for the SMALLER of the 16-byte path's and the
    scalar path's lane groups, whichever of the two the call then takes."""
    acc = 8 if elem_size == 8 else 4
    best = None
    for vec in (16 // elem_size, 1):
        nu = 256 // pick_group(-(-D // vec))
        cap = max(1, 48 * 1024 // (nu * (16 + 7 * acc)) - 1)
        best = cap if best is None else min(best, cap)
    return best


def fused_elem_size(storage):
    """the element size the limit is asked with: that of the ARITHMETIC type (16-bit storage next to float32 reference
    points keeps float32 records — compile_op.fused_lp_ok)"""
    return ARITH_BYTES[FUSED_ARITH[storage]]


def fused_case_list():
    """(family, storage, D, S): every D at S = 6, and S = 70 wherever the one-pass limit admits it.  That is every G = 32 and
    G = 64 class of the 16-byte path and the scalar path from two chunks on; a scalar-path D below that (17, 33; 65 in 16
    bits) is limited by the narrow group its 16-byte twin WOULD take (D = 17 in float32: 5 lanes, G = 8, 33 samples)."""
    out = []
    for family in FUSED_FAMILIES:
        for storage, dims in FUSED_DIMS.items():
            for D in dims:
                out.append((family, storage, D, FUSED_SMALL))
                if FUSED_LARGE <= fused_lp_limit(D, fused_elem_size(storage)):
                    assert instantiation(FUSED_ARITH[storage], D)[1] >= 32
                    out.append((family, storage, D, FUSED_LARGE))
    return out


def fused_ref_dims(family):
    return (4,) if family == "hfbox" else (2, 4)


def _fused_draw(family, storage, D, S, ref_dim, seed):
    import torch
    B, Q, H, levels = ec.HEAD_DIM_BASE
    L = len(levels)
    vdt, pdt, rdt = (getattr(torch, n) for n in FUSED_STORAGE[storage])
    g = torch.Generator(device="cpu").manual_seed(seed)
    big = torch.float64 if storage == "f64" else torch.float32
    ragged = family in ("ragged", "hfbox")
    counts = ([2, 4] if S == FUSED_SMALL else [30, 40]) if ragged else None
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=big).to(vdt)
    pshape = (B, Q, H, S, 3) if ragged else (B, Q, H, L, S // L, 3)
    proj = (torch.randn(pshape, generator=g, dtype=big) * 1.5).to(pdt)
    rshape = {"uniform": (B, Q, ref_dim), "ragged": (B, Q, ref_dim), "hfbox": (B, Q, 1, 4)}.get(family, (B, Q, L, ref_dim))
    ref = torch.rand(rshape, generator=g, dtype=big).to(rdt)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=big).to(pdt)
    mask = (torch.rand(B, value.shape[1], generator=g) < 0.5) if family == "levelref_masked" else None
    return dict(value=value, shapes=torch.tensor(levels), proj=proj, ref=ref, gout=gout, counts=counts, mask=mask,
                family=family, seed=seed)


def fused_sampling_inputs(family, proj, shapes, ref, counts):
    """The family's prologue in plain PyTorch (each pinned to the reference's / transformers' expression by the CPU suites)."""
    from msda_triton_amd import functional as F
    from msda_triton_amd.ragged import ragged_module_sampling_inputs
    if family == "uniform":
        return F.module_sampling_inputs(proj, shapes, ref)
    if family == "ragged":
        return ragged_module_sampling_inputs(proj, shapes, ref, counts)
    if family == "hfbox":
        return F.hf_box_sampling_inputs(proj, ref, counts, 0.5)
    return F.hf_module_sampling_inputs(proj, shapes, ref)


def _as_case(inp, pts, att, value):
    c = dict(value=value.numpy(), shapes=inp["shapes"].numpy(), loc=pts.detach().numpy(), attn=att.detach().numpy(),
             grad_out=inp["gout"].double().numpy(), bits=dict(loc=5))  # (bits: where `dense` puts its zero-weight padding)
    if inp["counts"] is not None:
        c["counts"] = inp["counts"]
    return c


def fused_kinks(inp, ac, tol=1e-4):
    """conftest.kink_mask on the float64 sampling points of the inputs as the kernels see them, in the projection's layout
    ([B, Q, H, L, P, 2] or [B, Q, H, S, 2])."""
    from conftest import kink_mask
    pts, att = fused_sampling_inputs(inp["family"], inp["proj"].double(), inp["shapes"], inp["ref"].double(), inp["counts"])
    c = _as_case(inp, pts, att, inp["value"].double())
    k = kink_mask(ec.dense(c)["loc"], c["shapes"], ac, tol)
    return ec._unpad(k, inp["counts"]) if inp["counts"] is not None else k



@functools.lru_cache(maxsize=None)
def fused_inputs(family, storage, D, S, ref_dim):
    """The case's inputs (host tensors in their storage types; cached, treat as read-only).  The seed is the first of the
    case's own sequence at which NO sample of either mode lies within 1e-4 of a grid kink: the reference points' gradients
    sum every sample's location gradient, a kink's jump included, so those are compared whole and want a kink-free draw."""
    import zlib
    base = zlib.crc32(f"{family} {storage} {D} {S} {ref_dim}".encode()) % 100000
    if storage not in FUSED_AGAINST_FP64:  # (16-bit inputs sit ON kinks; those results are held to the float32 kernels')
        return _fused_draw(family, storage, D, S, ref_dim, base)
    for k in range(256):
        inp = _fused_draw(family, storage, D, S, ref_dim, base + k)
        if not any(fused_kinks(inp, ac).any() for _, ac in FUSED_MODES):
            return inp
    raise AssertionError(f"no kink-free draw for {family} {storage} {D} {S} {ref_dim}")


def fused_reference(inp, pm, ac, oracle=None, real="float64"):
    """(out, grad_value, grad_proj, grad_ref) in float64 on the host — the prologue in PyTorch, the operator and its three
    gradients from the C oracle (per-level counts zero-padded to a dense layout, exact_cases.dense), the prologue's chain
    rule by autograd; with a value mask the oracle runs on where(mask, value, 0) and grad_value's padding rows are zero.
    real="float32": the same composition in float32 throughout (what the reference alone loses in that type)."""
    import numpy as np
    import torch
    tdt = getattr(torch, real)
    v64 = inp["value"].to(tdt)
    if inp["mask"] is not None:
        v64 = torch.where(inp["mask"][:, :, None, None], v64, torch.zeros_like(v64))
    p64, r64 = (inp[k].to(tdt).detach().clone().requires_grad_(True) for k in ("proj", "ref"))  # (never the cached tensors)
    pts, att = fused_sampling_inputs(inp["family"], p64, inp["shapes"], r64, inp["counts"])
    r = ec._oracle_all(oracle or ec._oracle(), _as_case(inp, pts, att, v64), pm, ac, getattr(np, real))
    gl, ga = (torch.from_numpy(np.ascontiguousarray(r[k])) for k in ("grad_loc", "grad_attn"))
    gp, gr = torch.autograd.grad([pts, att], [p64, r64], [gl, ga])
    gv = torch.from_numpy(r["grad_value"])
    if inp["mask"] is not None:
        gv = torch.where(inp["mask"][:, :, None, None], gv, torch.zeros_like(gv))
    return torch.from_numpy(r["out"]), gv, gp, gr


# ----------------------------------------------------------------------------------------- the fused families ON the lattice
# Points the prologues form EXACTLY in float32, in either order of operations (offset / w or offset * (1 / w)): the offset
# is zero, or every factor it meets is a power of two — the level sizes of exact_cases.LATTICE_LEVELS[False], point counts
# of 1, 2, 4, box sizes of 1/4, 1/2, 1 — and reference points and offsets are short dyadic numbers.  The kernels, the
# float32 composition and the float64 reference then sample the SAME points, on the same side of every kink, and the
# location gradients can be compared with no sample masked out.  align_corners with 2-d reference points divides the
# offsets by 2^k + 1: those draws have zero offsets (the zero-initialised module) and put the reference points themselves
# on the lattice.
LATTICE_B, LATTICE_Q, LATTICE_H = 2, 384, 2
LATTICE_P, LATTICE_COUNTS = 2, [2, 4, 1, 1]
LATTICE_FUSED_DIMS = {"f32": (32, 5), "f64": (32, 5), "bf16": (32,), "fp16": (32,), "sbf16": (32,), "sf16": (32,),
                      "vbf16": (32,), "vf16": (32,)}
LATTICE_FUSED_MODES = ec.MODES
# ... and the universal values on arbitrary sizes (exact_cases.UNIVERSAL_LEVELS): with 2-d reference points the
# zero-initialised module on reference points out of a clamp(0, 1) — 0, 0.5, 1 and -0 —, with boxes (whose rule knows no
# level size) offsets that put every sample on one of those values or a dyadic neighbour; one 16-byte D per arithmetic
UNIVERSAL_COUNTS = [2, 4, 1]
UNIVERSAL_FUSED_DIMS = {"f32": (32,), "f64": (32,), "sbf16": (32,), "bf16": (32,)}


def fused_lattice_case_list():
    """(family, storage, D, ref_dim, universal)"""
    return [(f, s, d, rd, u) for u, table in ((False, LATTICE_FUSED_DIMS), (True, UNIVERSAL_FUSED_DIMS)) for f in FUSED_FAMILIES
            for s, dims in table.items() for d in dims for rd in fused_ref_dims(f)]


@functools.lru_cache(maxsize=None)
def fused_lattice_inputs(family, storage, D, ref_dim, ac, universal=False):
    """The inputs of `_fused_draw` (host tensors in their storage types; cached, read-only) with offsets and reference
    points such that the family's prologue lands on the lattice targets of `exact_cases.lattice_case` — the full lattice
    of align_corners = ac, or the universal values on UNIVERSAL_LEVELS — plus "points" (the float64 sampling points, the
    family's layout) and "factor" (what the prologue multiplies the offsets by, float64)."""
    import zlib
    import numpy as np
    import torch
    B, Q, H = LATTICE_B, LATTICE_Q, LATTICE_H
    levels = ec.UNIVERSAL_LEVELS if universal else ec.LATTICE_LEVELS[ac]
    align = None if universal else ac
    L = len(levels)
    ragged = family in ("ragged", "hfbox")
    perlevel = family in ("levelref", "levelref_masked")
    counts = (UNIVERSAL_COUNTS if universal else LATTICE_COUNTS) if ragged else None
    per = counts if ragged else [LATTICE_P] * L
    S = sum(per)
    seed = zlib.crc32(f"lattice {family} {ref_dim} {ac} {universal}".encode()) % 100000  # (one draw of points for every storage and D)
    rng = np.random.default_rng(seed)
    vdt, pdt, rdt = (getattr(torch, n) for n in FUSED_STORAGE[storage])
    g = torch.Generator(device="cpu").manual_seed(seed)
    big = torch.float64 if storage == "f64" else torch.float32
    value = torch.randn(B, sum(h * w for h, w in levels), H, D, generator=g, dtype=big).to(vdt)
    logits = (torch.randn((B, Q, H, S), generator=g, dtype=big) * 1.5).to(pdt)
    gout = torch.rand(B, Q, H, D, generator=g, dtype=big).to(pdt)
    mask = (torch.rand(B, value.shape[1], generator=g) < 0.5) if family == "levelref_masked" else None
    # targets [B, Q, H, S, 2], level-major, and each sample's level
    target = ec.lattice_case(rng, B, Q, H, 1, levels, per, align=align)["loc"]
    level = np.repeat(np.arange(L), per)
    hw = np.asarray(levels, dtype=np.float64)[level]              # [S, 2] (h, w)
    pl = np.asarray(per, dtype=np.float64)[level][:, None]         # [S, 1] the count of the sample's level
    zero_offsets = (universal or bool(ac)) and ref_dim == 2        # offsets divided by 2^k + 1 (or any) pixels: none
    # reference points [B, Q, (L,) ref_dim]
    rshape = (B, Q, L) if perlevel else (B, Q)
    if zero_offsets:  # the reference points ARE the sampling points: a level's own lattice (per-level), level 0's otherwise
        own = ec.lattice_case(rng, B, Q, 1, 1, levels, 1, align=align)["loc"][:, :, 0, :, 0]  # [B, Q, L, 2]: every pair, per level
        xy = own if perlevel else own[:, :, 0]
    else:
        xy = rng.integers(0, 17, size=rshape + (2,)) / 16.0
    ref = xy if ref_dim == 2 else np.concatenate([xy, rng.choice([0.25, 0.5, 1.0], size=rshape + (2,))], -1)
    rs = ref[:, :, None, level] if perlevel else ref[:, :, None, None]   # -> [B, Q, 1, S, ref_dim] per sample
    if ref_dim == 2:
        # (the reference module and its per-level-count form divide (x, y) by the stored (h, w); transformers by (w, h))
        factor = 1.0 / (hw[:, ::-1] if perlevel else hw) * np.ones((B, Q, 1, S, 2))
    else:
        factor = rs[..., 2:] / (2.0 * pl)
    offsets = np.zeros((B, Q, H, S, 2)) if zero_offsets else (target - rs[..., :2]) / factor
    points = rs[..., :2] + offsets * factor
    assert zero_offsets or np.array_equal(points, target)
    proj = torch.cat([torch.from_numpy(offsets).to(pdt), logits[..., None]], -1)
    if family == "hfbox":
        ref = ref[:, :, None]
    if not ragged:
        proj, points, factor = (t.reshape((B, Q, -1, L, LATTICE_P) + tuple(t.shape[4:])) for t in (proj, points, factor))
    return dict(value=value, shapes=torch.tensor(levels), proj=proj, ref=torch.from_numpy(ref).to(rdt), gout=gout, counts=counts,
                mask=mask, family=family, seed=seed, points=points, factor=factor, zero_offsets=zero_offsets)
