"""Precise RoI Pooling restated in differentiable torch (a test helper, not an oracle module).

The pooled value of a bin is the integral of the bilinear surface through the feature samples over the bin, divided by
the bin's area.  The surface is a sum of products of hat functions, so the integral separates per axis: sample p of an
axis weighs G(e - p) - G(s - p) in a window [s, e], G being the hat's antiderivative (closed form, below).  Everything
is built from tensor ops in the dtype of `feat`, so autograd yields the gradient to the features and to the boxes, and
the same code runs in float64 (the reference of the tests) and in float32 on the CPU (whose error against float64
sets the bars of the GPU tests).  Samples outside the map are zero, as in the reference's kernels; the ROI rules are
the operator's (include/mmtrack.h): a ROI with a non-finite value, an index outside [0, N), a geometry that overflows
float32, or no area pools to zeros with zero gradients.

There is no reference binary to compare with (the reference's extension is CUDA only): the operator is pinned to this
restatement, to the reference's own known-answer property (integer-aligned ROIs equal avg_pool2d(2, 1) slices) and to
finite differences (tests/test_prroi_ref.py).
"""
import torch


def _hat_antiderivative(u):
    """G(u) = integral of max(0, 1 - |t|) from -inf to u: 0 below -1, (u + 1)^2 / 2 on [-1, 0], 1/2 + u - u^2 / 2 on
    [0, 1], 1 above."""
    u = u.clamp(-1.0, 1.0)
    return 0.5 + u - 0.5 * u * u.abs()


def _geometry(r, scale, ph, pw):
    x0, y0 = r[:, 1] * scale, r[:, 2] * scale
    bw = (r[:, 3] * scale - x0).clamp(min=0) / pw
    bh = (r[:, 4] * scale - y0).clamp(min=0) / ph
    return x0, y0, bw, bh, bw * bh


def prroi_pool_ref(feat, rois, ph, pw, scale):
    """feat [N, C, H, W]; rois [K, 5] = (batch index, x0, y0, x1, y1) -> [K, C, ph, pw], in feat's dtype."""
    N, C, H, W = feat.shape
    K = rois.shape[0]
    dt = feat.dtype
    if K == 0:
        return feat.new_zeros((0, C, ph, pw))
    r = rois.to(dt)
    with torch.no_grad():                                  # the operator's rules, in the operator's float32
        rf = rois.float()
        ok = torch.isfinite(rf).all(1) & (rf[:, 0] >= 0) & (rf[:, 0] < N)
        geo = _geometry(rf, scale, ph, pw)
        for v in geo:
            ok = ok & torch.isfinite(v)
        ok = ok & (geo[4] > 0)
    dummy = torch.tensor([0.0, 0.0, 0.0, 1.0 / scale, 1.0 / scale], dtype=dt)
    r = torch.where(ok[:, None], r, dummy)                 # a ROI that pools to zeros takes no part in autograd
    x0, y0, bw, bh, area = _geometry(r, scale, ph, pw)
    n = r[:, 0].detach().long()
    j = torch.arange(pw, dtype=dt)
    i = torch.arange(ph, dtype=dt)
    ws = x0[:, None] + bw[:, None] * j                     # [K, pw]
    hs = y0[:, None] + bh[:, None] * i                     # [K, ph]
    px = torch.arange(W, dtype=dt)
    py = torch.arange(H, dtype=dt)
    wx = _hat_antiderivative((ws + bw[:, None])[:, :, None] - px) - _hat_antiderivative(ws[:, :, None] - px)
    wy = _hat_antiderivative((hs + bh[:, None])[:, :, None] - py) - _hat_antiderivative(hs[:, :, None] - py)
    out = torch.einsum("kih,kjw,kchw->kcij", wy, wx, feat[n]) / area[:, None, None, None]
    return out * ok[:, None, None, None].to(dt)


def gradients(feat, rois, ph, pw, scale, grad_out):
    """(out, grad_feat, grad_rois) of sum(out * grad_out), in feat's dtype."""
    f = feat.clone().requires_grad_(True)
    r = rois.clone().requires_grad_(True)
    out = prroi_pool_ref(f, r, ph, pw, scale)
    if out.numel() == 0:
        return out.detach(), torch.zeros_like(feat), torch.zeros_like(rois)
    gf, gr = torch.autograd.grad((out * grad_out.to(out.dtype)).sum(), (f, r), allow_unused=True)
    gr = torch.zeros_like(rois) if gr is None else torch.nan_to_num(gr, nan=0.0)
    return out.detach(), gf, gr


INF, NAN = float("inf"), float("nan")


def adversarial_rois(N):
    """ROIs no kernel may trip over, as (index, x0, y0, x1, y1) in map cells (spatial scale 1), and whether each is
    valid (pools to something): bad indices, non-finite and huge coordinates, no or negative extent, integer-aligned
    edges."""
    rows = [
        ([-1.0, 1.0, 1.0, 3.0, 3.0], False), ([float(N), 1.0, 1.0, 3.0, 3.0], False),
        ([1e9, 1.0, 1.0, 3.0, 3.0], False), ([NAN, 1.0, 1.0, 3.0, 3.0], False),
        ([0.0, -INF, 1.0, 3.0, 3.0], False), ([0.0, 1.0, 1.0, INF, 3.0], False),
        ([0.0, 1.0, NAN, 3.0, 3.0], False), ([1.0, 1.0, 1.0, 3.0, -INF], False),
        ([0.0, -1e30, -1e30, 1e30, 1e30], False),           # the bin area overflows float32
        ([0.0, -1e30, 1.0, 1e30, 3.0], True),               # 2e30 wide, 2 high: finite geometry, pools to ~0
        ([1.0, -5e8, 0.5, 5e8, 2.5], True),                 # 1e9 wide
        ([0.0, 2.0, 1.0, 2.0, 3.0], False), ([0.0, 1.0, 2.0, 3.0, 2.0], False),   # zero extent
        ([1.0, 3.0, 1.0, 1.0, 3.0], False), ([1.0, 1.0, 3.0, 3.0, 1.0], False),   # negative extent
        ([0.0, 0.0, 0.0, 4.0, 4.0], True), ([1.0, 1.0, 2.0, 3.0, 4.0], True),     # integer-aligned edges
        ([0.9999, 0.5, 0.5, 2.5, 2.5], True),               # the index truncates to 0
    ]
    return torch.tensor([r for r, _ in rows], dtype=torch.float32), [v for _, v in rows]
