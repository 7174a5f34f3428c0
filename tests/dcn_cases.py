"""Cases and the float64 reference of the deformable convolution core (DCNv3 / DCNv4), for test_dcn.py and test_gpu_dcn.py.

The reference is explicit index arithmetic — floor, four corners, a gather by indexing, zero outside the image — written
from the operator's statement; it shares no code with the package's formulation and does not use grid_sample.  Autograd
differentiates it for the three gradients.  Offsets are drawn from N(0, 1.5^2): taps cross every border."""
import torch

NAMES = ("out", "grad_input", "grad_offset", "grad_mask")
BASE = dict(N=2, Hi=5, Wi=7, G=3, D=4, kernel=(3, 3), stride=(1, 1), pad=(1, 1), dil=(1, 1), scale=1.0, softmax=False)
F64 = torch.float64


def out_size(Hi, Wi, kernel, stride, pad, dil):
    return tuple((n + 2 * p - (d * (k - 1) + 1)) // s + 1 for n, k, s, p, d in zip((Hi, Wi), kernel, stride, pad, dil))


def reference(inp, offset, mask, kernel, stride, pad, dil, scale, softmax):
    """inp [N, Hi, Wi, G, D], offset [N, Ho, Wo, G, K, 2] (x, y), mask [N, Ho, Wo, G, K], all float64 -> [N, Ho, Wo, G, D]."""
    N, Hi, Wi, G, D = inp.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = kernel, stride, pad, dil
    Ho, Wo = out_size(Hi, Wi, kernel, stride, pad, dil)
    cx, cy = (dw * (kw - 1)) // 2, (dh * (kh - 1)) // 2
    m = mask.softmax(-1) if softmax else mask
    out = inp.new_zeros((N, Ho, Wo, G, D))
    n_idx = torch.arange(N).view(N, 1, 1, 1).expand(N, Ho, Wo, G)
    g_idx = torch.arange(G).view(1, 1, 1, G).expand(N, Ho, Wo, G)
    ho = torch.arange(Ho, dtype=F64).view(1, Ho, 1, 1)
    wo = torch.arange(Wo, dtype=F64).view(1, 1, Wo, 1)
    for i in range(kw):      # the window's column: the OUTER index
        for j in range(kh):  # its row
            k = i * kh + j
            lx = wo * sw - pw + cx + scale * (i * dw - cx + offset[..., k, 0])
            ly = ho * sh - ph + cy + scale * (j * dh - cy + offset[..., k, 1])
            x0, y0 = lx.detach().floor(), ly.detach().floor()
            fx, fy = lx - x0, ly - y0
            for cyy, cxx, w in ((y0, x0, (1 - fy) * (1 - fx)), (y0, x0 + 1, (1 - fy) * fx),
                                (y0 + 1, x0, fy * (1 - fx)), (y0 + 1, x0 + 1, fy * fx)):
                inside = (cxx >= 0) & (cxx <= Wi - 1) & (cyy >= 0) & (cyy <= Hi - 1)
                rows = inp[n_idx, cyy.clamp(0, Hi - 1).long(), cxx.clamp(0, Wi - 1).long(), g_idx]  # [N, Ho, Wo, G, D]
                out = out + (m[..., k] * w * inside)[..., None] * rows
    return out


def make_inputs(dtype=F64, seed=0, offset_std=1.5, **over):
    """The case's inputs, rounded to `dtype` and held in float64 (so the reference sees what the kernels see)."""
    c = dict(BASE, **over)
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(c["Hi"], c["Wi"], c["kernel"], c["stride"], c["pad"], c["dil"])
    K = c["kernel"][0] * c["kernel"][1]
    shapes = dict(input=(c["N"], c["Hi"], c["Wi"], c["G"], c["D"]), offset=(c["N"], Ho, Wo, c["G"], K, 2),
                  mask=(c["N"], Ho, Wo, c["G"], K), grad_out=(c["N"], Ho, Wo, c["G"], c["D"]))
    t = {name: torch.randn(shape, generator=g, dtype=F64) for name, shape in shapes.items()}
    t["offset"] = t["offset"] * offset_std
    return c, {name: v.to(dtype).to(F64) for name, v in t.items()}


def run(fn, c, inputs, dtype=F64, device="cpu", needs=(True, True, True), **kw):
    """fn(input, offset, mask, kernel, stride, pad, dil, scale, softmax) forward + backward -> {name: float64 on the CPU}."""
    leaves = [inputs[n].to(device=device, dtype=dtype, copy=True).requires_grad_(need) for n, need in zip(("input", "offset", "mask"), needs)]
    out = fn(*leaves, c["kernel"], c["stride"], c["pad"], c["dil"], c["scale"], c["softmax"], **kw)
    out.backward(inputs["grad_out"].to(device=device, dtype=dtype))
    res = [out.detach()] + [t.grad for t in leaves]
    return {name: None if v is None else v.detach().to("cpu", F64) for name, v in zip(NAMES, res)}


_WANT = {}


def case(dtype=F64, seed=0, offset_std=1.5, **over):
    """(settings, inputs, the reference's results) — computed once per case and shared."""
    key = (dtype, seed, offset_std, tuple(sorted(over.items())))
    if key not in _WANT:
        c, inputs = make_inputs(dtype, seed, offset_std, **over)
        _WANT[key] = (c, inputs, run(reference, c, inputs))
    return _WANT[key]


def assert_close(got, want, fwd_tol, bwd_tol, label=""):
    for name in NAMES:
        if got[name] is not None:
            torch.testing.assert_close(got[name], want[name], **(fwd_tol if name == "out" else bwd_tol),
                                       msg=lambda m, n=name: f"{label}{n}: {m}")
