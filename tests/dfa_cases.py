"""Cases and the float64 reference of deformable feature aggregation, for test_dfa.py and test_gpu_dfa.py.

The reference is explicit index arithmetic — validity, floor, four corners, a gather by indexing, zero outside the map —
written from the operator's statement in include/msda_hip.h; it shares no code with the package's formulation and does not
use grid_sample.  Autograd differentiates it for the three gradients."""
import torch

NAMES = ("out", "grad_feature_maps", "grad_sampling_locations", "grad_weights")
SHAPES = (((5, 7), (3, 4)), ((4, 6), (2, 3)), ((6, 5), (3, 3)))  # [cams][levels] (h, w): every camera its own size
BASE = dict(B=2, A=5, P=3, G=2, D=4, shapes=SHAPES)
F64 = torch.float64


def reference(fm, shapes, loc, wts):
    """fm [B, I, G, D], shapes [cams, levels, 2], loc [B, A, P, cams, 2] (x, y), wts [B, A, P, cams, levels, G] -> [B, A, G, D]."""
    B, A, P, cams, levels, G = wts.shape
    valid = ((loc > 0) & (loc < 1)).all(-1)  # [B, A, P, cams]
    out = fm.new_zeros((B, A, G, fm.shape[3]))
    b_idx = torch.arange(B).view(B, 1, 1)
    start = 0
    for c, cam_shapes in enumerate(shapes.tolist()):
        for l, (h, w) in enumerate(cam_shapes):  # noqa: E741
            px, py = loc[..., c, 0] * w - 0.5, loc[..., c, 1] * h - 0.5
            x0, y0 = px.detach().floor(), py.detach().floor()
            fx, fy = px - x0, py - y0
            for cy, cx, k in ((y0, x0, (1 - fy) * (1 - fx)), (y0, x0 + 1, (1 - fy) * fx),
                              (y0 + 1, x0, fy * (1 - fx)), (y0 + 1, x0 + 1, fy * fx)):
                inside = (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1) & valid[..., c]
                rows = fm[b_idx, start + cy.clamp(0, h - 1).long() * w + cx.clamp(0, w - 1).long()]  # [B, A, P, G, D]
                out = out + ((wts[:, :, :, c, l] * (k * inside)[..., None])[..., None] * rows).sum(2)
            start += h * w
    return out


def expansion(fm, shapes, loc, wts):
    """The operator through multiscale_deformable_attention: L = cams * levels, the location broadcast over levels and groups,
    the validity mask multiplied into the weights."""
    from msda_triton_amd import multiscale_deformable_attention
    B, A, P, cams, levels, G = wts.shape
    valid = ((loc > 0) & (loc < 1)).all(-1).to(wts.dtype)
    points = loc.permute(0, 1, 3, 2, 4)[:, :, None, :, None].expand(B, A, G, cams, levels, P, 2).reshape(B, A, G, cams * levels, P, 2)
    attn = (wts * valid[..., None, None]).permute(0, 1, 5, 3, 4, 2).reshape(B, A, G, cams * levels, P)
    return multiscale_deformable_attention(fm, shapes.reshape(-1, 2), points, attn, "zeros", False)


def make_inputs(dtype=F64, seed=0, exact=False, **over):
    """The case's inputs, rounded to `dtype` and held in float64 (so the reference sees what the kernels see)."""
    c = dict(BASE, **over)
    g = torch.Generator().manual_seed(seed)
    B, A, P, G, D = (c[k] for k in "BAPGD")
    shapes = torch.tensor(c["shapes"], dtype=torch.int64)
    cams, levels = shapes.shape[:2]
    I = int(shapes.prod(-1).sum())  # noqa: E741
    if exact:  # small integers, ones, pixel centres of every camera's first level: every product and sum is exact
        t = dict(fm=torch.randint(-8, 9, (B, I, G, D), generator=g).to(F64), wts=torch.ones(B, A, P, cams, levels, G, dtype=F64),
                 grad_out=torch.randint(-8, 9, (B, A, G, D), generator=g).to(F64))
        hw = shapes[:, 0].to(F64).flip(-1)  # [cams, (w, h)]
        t["loc"] = ((torch.rand(B, A, P, cams, 2, generator=g, dtype=F64) * hw).floor() + 0.5) / hw
    else:
        t = dict(fm=torch.randn(B, I, G, D, generator=g, dtype=F64), wts=torch.randn(B, A, P, cams, levels, G, generator=g, dtype=F64),
                 grad_out=torch.randn(B, A, G, D, generator=g, dtype=F64),
                 loc=torch.rand(B, A, P, cams, 2, generator=g, dtype=F64) * 1.5 - 0.25)
        loc = t["loc"]
        if A >= 5 and P >= 3 and B >= 2:  # planted: the strict bounds, partial corners, a camera and an anchor out of view
            loc[0, 0, 0, 0] = torch.tensor([0.0, 0.5], dtype=F64)
            loc[0, 0, 1, 0] = torch.tensor([0.5, 1.0], dtype=F64)
            loc[0, 1, 0, :] = torch.tensor([0.02, 0.98], dtype=F64)
            loc[0, 1, 1, :] = torch.tensor([0.99, 0.01], dtype=F64)
            loc[0, 2, :, 1] = 1.2
            loc[1, 3] = -0.1
    return c, shapes, {name: v.to(dtype).to(F64) for name, v in t.items()}


def run(fn, shapes, inputs, dtype=F64, device="cpu", needs=(True, True, True)):
    """fn(feature_maps, spatial_shapes, sampling_locations, weights) forward + backward -> {name: float64 on the CPU}."""
    leaves = [inputs[n].to(device=device, dtype=dtype, copy=True).requires_grad_(need) for n, need in zip(("fm", "loc", "wts"), needs)]
    out = fn(leaves[0], shapes.to(device), leaves[1], leaves[2])
    out.backward(inputs["grad_out"].to(device=device, dtype=dtype))
    res = [out.detach()] + [t.grad for t in leaves]
    return {name: None if v is None else v.detach().to("cpu", F64) for name, v in zip(NAMES, res)}


_WANT = {}


def case(dtype=F64, seed=0, exact=False, **over):
    """(spatial_shapes, inputs, the reference's results) — computed once per case and shared."""
    key = (dtype, seed, exact, tuple(sorted(over.items())))
    if key not in _WANT:
        c, shapes, inputs = make_inputs(dtype, seed, exact, **over)
        if not exact:  # neither an all-valid nor an all-dropped draw can pass for coverage
            loc = inputs["loc"]
            dropped = 1 - ((loc > 0) & (loc < 1)).all(-1).double().mean().item()
            assert 0.3 <= dropped <= 0.7, dropped
        _WANT[key] = (shapes, inputs, run(reference, shapes, inputs))
    return _WANT[key]


def assert_close(got, want, fwd_tol, bwd_tol, label=""):
    for name in NAMES:
        if got[name] is not None:
            torch.testing.assert_close(got[name], want[name], **(fwd_tol if name == "out" else bwd_tol),
                                       msg=lambda m, n=name: f"{label}{n}: {m}")
