"""Inputs and the float64 reference of the key-aware attention tests (test_key_aware.py, test_gpu_key_aware.py).

The reference is the operator's definition in plain PyTorch on the CPU in float64 — index arithmetic and ``gather``, no
``grid_sample``, nothing of the package — and its gradients are autograd's."""
import functools

import torch

BASE_LEVELS = ((5, 7), (3, 2), (1, 1))
MODES = [("border", False), ("border", True), ("zeros", False), ("zeros", True)]
NAMES = ("out", "attn", "grad_query", "grad_key", "grad_value", "grad_points")


def _bilinear(plane, pts, h, w, pm, ac):
    """plane [B, H, h*w, D], pts [B, H, Q, P, 2] -> [B, H, Q, P, D]"""
    B, H, _, D = plane.shape
    Q, P = pts.shape[2:4]
    total = 0
    pix = []
    for c, n in ((0, w), (1, h)):
        v = pts[..., c] * (n - 1) if ac else pts[..., c] * n - 0.5
        if pm == "border":  # clipped to the edge pixel, and no gradient at or beyond it
            v = torch.where((v > 0) & (v < n - 1), v, v.detach().clamp(0, n - 1))
        pix.append(v)
    (px, py), (x0, y0) = pix, (pix[0].detach().floor(), pix[1].detach().floor())
    dx, dy = px - x0, py - y0
    for yo, xo, wgt in ((0, 0, (1 - dy) * (1 - dx)), (0, 1, (1 - dy) * dx), (1, 0, dy * (1 - dx)), (1, 1, dy * dx)):
        xi, yi = x0 + xo, y0 + yo
        valid = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long().reshape(B, H, Q * P, 1).expand(-1, -1, -1, D)
        total = total + plane.gather(2, idx).reshape(B, H, Q, P, D) * (wgt * valid).unsqueeze(-1)
    return total


def reference(query, key, value, levels, points, pm, ac, scale):
    """-> (out [B, Q, H, D], attn [B, Q, H, L, P]) in the inputs' dtype (float64 in the tests)"""
    B, Q, H, D = query.shape
    L, P = points.shape[3:5]
    ks, vs, start = [], [], 0
    for lvl, (h, w) in enumerate(levels):
        pts = points[:, :, :, lvl].permute(0, 2, 1, 3, 4)
        for src, dst in ((key, ks), (value, vs)):
            dst.append(_bilinear(src.permute(0, 2, 1, 3)[:, :, start:start + h * w], pts, h, w, pm, ac))
        start += h * w
    ks, vs = torch.cat(ks, 3), torch.cat(vs, 3)  # [B, H, Q, L*P, D]
    attn = (scale * (query.permute(0, 2, 1, 3).unsqueeze(3) * ks).sum(-1)).softmax(-1)
    out = (attn.unsqueeze(-1) * vs).sum(3)
    return out.permute(0, 2, 1, 3), attn.reshape(B, H, Q, L, P).permute(0, 2, 1, 3, 4)


@functools.lru_cache(maxsize=None)
def case(B=2, H=3, Q=37, D=32, levels=BASE_LEVELS, P=2, dtype=torch.float32, seed=0, pm="border", ac=False, peaked=False):
    """Inputs (float64, rounded to ``dtype`` first) and the reference results, computed once per case and shared:
    ``(inputs dict, results dict by NAMES)``.  Points are uniform in [-0.1, 1.1]^2: both padding edges are hit.
    ``peaked``: query = 8 |q| and the unit's LAST sample sits on the last level's first pixel, whose key row is the largest — the
    running maximum of an online softmax moves on the last sample."""
    g = torch.Generator().manual_seed(seed)
    I, L = sum(h * w for h, w in levels), len(levels)  # noqa: E741
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    query, key, value, grad_out = rnd(B, Q, H, D), rnd(B, I, H, D), rnd(B, I, H, D), rnd(B, Q, H, D)
    points = torch.rand(B, Q, H, L, P, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1
    if peaked:
        h_l, w_l = levels[-1]
        query = 8 * query.abs()
        key[:, I - h_l * w_l] = 3.0
        points[:, :, :, L - 1, P - 1] = torch.tensor([0.6 / w_l, 0.6 / h_l], dtype=torch.float64)
    inputs = {k: v.to(dtype).double() for k, v in dict(query=query, key=key, value=value, points=points, grad_out=grad_out).items()}
    leaves = [inputs[k].clone().requires_grad_(True) for k in ("query", "key", "value", "points")]
    out, attn = reference(*leaves[:3], levels, leaves[3], pm, ac, D ** -0.5)
    grads = torch.autograd.grad(out, leaves, inputs["grad_out"])
    return inputs, dict(zip(NAMES, (out.detach(), attn.detach()) + grads))


def run(fn, inputs, levels, pm, ac, dtype, device, needs=(True, True, True, True), pyramids=None):
    """``fn`` = key_aware_deformable_attention on the case's inputs in ``dtype`` on ``device`` -> results dict by NAMES
    (None for a tensor not in ``needs``: query, key, value, points).  ``pyramids``: (key, value) tensors to use instead."""
    q, k, v, p = (inputs[n].to(dtype).to(device) for n in ("query", "key", "value", "points"))
    if pyramids is not None:
        k, v = pyramids
    leaves = [t.requires_grad_(n) for t, n in zip((q, k, v, p), needs)]
    shapes = torch.tensor(levels, dtype=torch.int64, device=device)
    out, attn = fn(leaves[0], leaves[1], leaves[2], shapes, leaves[3], pm, ac, return_attention=True)
    wrt = [t for t, n in zip(leaves, needs) if n]
    grads = iter(torch.autograd.grad(out, wrt, inputs["grad_out"].to(dtype).to(device)))
    return dict(zip(NAMES, (out.detach(), attn) + tuple(next(grads) if n else None for n in needs)))


def assert_close(got, want, fwd_tol, bwd_tol):
    """every element of every result against the float64 reference"""
    for name in NAMES:
        tol = fwd_tol if name in ("out", "attn") else bwd_tol
        print(name, "max abs err", float((got[name].double().cpu() - want[name]).abs().max()))
        torch.testing.assert_close(got[name].double().cpu(), want[name], **tol, msg=lambda m, n=name: f"{n}: {m}")
