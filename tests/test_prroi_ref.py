"""tests/prroi_ref.py, the differentiable restatement the PrRoIPool kernels are tested against, checked on the CPU:
against the oracle's forward, against central differences, against the reference's own known-answer property and on
ROIs that must pool to zeros."""
import math

import torch
import torch.nn.functional as F

from oracle import dimpnet as odn
from tests.prroi_ref import adversarial_rois, gradients, prroi_pool_ref


def test_matches_oracle_forward_on_one_roi_per_image():
    """(a) oracle.dimpnet.prroi_pool evaluates its cell weights and the final division in float32, so it equals a
    float64 evaluation to 1e-12 only where float32 is exact.  The inputs make it so: features are multiples of 1/16
    below 4, ROI starts multiples of 1/4 and bin sizes 1/2, 1 or 2 cells, so every weight is a multiple of 2^-14
    below 1, every cell sum fits 24 bits and every bin area is a power of two."""
    g = torch.Generator().manual_seed(3)
    N, C, H, W = 6, 3, 7, 9
    feat = torch.randint(-63, 64, (N, C, H, W), generator=g).double() / 16
    for ph, pw, scale in ((4, 4, 1 / 16), (2, 3, 1 / 8)):
        cells = torch.tensor([   # x0, y0 in cells, bin width, bin height in cells
            [1.25, 0.5, 1.0, 0.5], [0.0, 0.0, 2.0, 1.0], [-1.5, -0.75, 1.0, 1.0], [5.25, 3.5, 2.0, 2.0],
            [2.0, 3.0, 0.5, 0.5], [-8.0, -8.0, 1.0, 1.0]], dtype=torch.float64)
        rois = torch.zeros(N, 5, dtype=torch.float64)
        rois[:, 0] = torch.arange(N)
        rois[:, 1], rois[:, 2] = cells[:, 0] / scale, cells[:, 1] / scale
        rois[:, 3] = (cells[:, 0] + cells[:, 2] * pw) / scale
        rois[:, 4] = (cells[:, 1] + cells[:, 3] * ph) / scale
        want = odn.prroi_pool(feat.float(), rois.float(), scale, ph, pw).double()
        got = prroi_pool_ref(feat, rois, ph, pw, scale)
        assert want.abs().max() > 0.5
        assert (got - want).abs().max() <= 1e-12


def _smooth_rois(N, H, W, ph, pw, scale, K, seed):
    """Random ROIs across and inside the map whose every bin edge lies at least 0.05 cells from an integer."""
    g = torch.Generator().manual_seed(seed)
    rois = []
    while len(rois) < K:
        x0 = (torch.rand(1, generator=g).item() * (W + 1) - 1.5)
        y0 = (torch.rand(1, generator=g).item() * (H + 1) - 1.5)
        bw = 0.3 + torch.rand(1, generator=g).item() * 1.5
        bh = 0.3 + torch.rand(1, generator=g).item() * 1.5
        edges = [x0 + bw * j for j in range(pw + 1)] + [y0 + bh * i for i in range(ph + 1)]
        if min(abs(e - round(e)) for e in edges) < 0.06:
            continue
        rois.append([float(len(rois) % N), x0 / scale, y0 / scale, (x0 + bw * pw) / scale, (y0 + bh * ph) / scale])
    return torch.tensor(rois, dtype=torch.float64)


def test_box_gradient_matches_central_differences():
    """(b) With every bin edge off the integers the pooled value is smooth in the box, and along one coordinate t it is
    A(t) / b(t) per axis: A, the weighted sample sum, is quadratic in t on the smooth piece (the weights are differences
    of the piecewise-quadratic G), and b, the bin size, is affine with |b'| = s / P (s the spatial scale, P the bins of
    the axis).  With F = max |feat|: |A| <= b F, |A'| <= 2 s F (the hats at an edge sum to 1, two edges), |A''| <=
    4 s^2 F, and with q = 1 / (ROI extent in image units) = |b'| / b the derivatives of 1 / b are q / b, 2 q^2 / b,
    6 q^3 / b, so |(A / b)'''| <= F (12 s^2 q / b + 12 s q^2 / b + 6 q^3).  The other axis is an average (factor <= 1).
    A central difference of step h is off by at most h^2 / 6 times that, summed over the ROI's outputs with
    |grad_out|, plus the float64 rounding of the two evaluations, taken as 64 ulp of sum |grad_out| F over h."""
    N, C, H, W, ph, pw, scale, h = 2, 3, 6, 8, 3, 2, 0.25, 1e-3
    g = torch.Generator().manual_seed(11)
    feat = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    rois = _smooth_rois(N, H, W, ph, pw, scale, 8, seed=5)
    # the test's own inputs: every bin edge at least 0.05 cells from an integer, and h moves an edge far less
    for r in rois:
        edges = [r[1] * scale + (r[3] - r[1]) * scale * j / pw for j in range(pw + 1)]
        edges += [r[2] * scale + (r[4] - r[2]) * scale * i / ph for i in range(ph + 1)]
        assert min(abs(float(e) - round(float(e))) for e in edges) >= 0.05
    assert h * scale < 0.005
    gout = torch.randn(rois.shape[0], C, ph, pw, generator=g, dtype=torch.float64)
    _, _, grad = gradients(feat, rois, ph, pw, scale, gout)
    assert torch.equal(grad[:, 0], torch.zeros(rois.shape[0], dtype=torch.float64))
    Fm = float(feat.abs().max())
    worst = 0.0
    for k in range(rois.shape[0]):
        gsum = float(gout[k].abs().sum())
        for col in (1, 2, 3, 4):
            P = pw if col in (1, 3) else ph
            ext = float(rois[k, 3] - rois[k, 1]) if col in (1, 3) else float(rois[k, 4] - rois[k, 2])
            ext -= h                                     # the smallest extent the two evaluations see
            q, b = 1.0 / ext, ext * scale / P
            third = Fm * (12 * scale ** 2 * q / b + 12 * scale * q ** 2 / b + 6 * q ** 3)
            tol = h * h / 6 * third * gsum + 64 * 2.3e-16 * gsum * Fm / h
            plus, minus = rois.clone(), rois.clone()
            plus[k, col] += h
            minus[k, col] -= h
            fd = ((prroi_pool_ref(feat, plus, ph, pw, scale)[k] - prroi_pool_ref(feat, minus, ph, pw, scale)[k])
                  * gout[k]).sum() / (2 * h)
            err = abs(float(fd) - float(grad[k, col]))
            worst = max(worst, err / tol)
            assert err <= tol, (k, col, err, tol, float(fd), float(grad[k, col]))
    assert float(grad[:, 1:].abs().max()) > 1e-2         # not a comparison of zeros
    print(f"largest central-difference error / derived bound: {worst:.3g}")


def test_integer_aligned_rois_equal_avg_pool():
    """(c) The reference's unit-test property (pytorch/tests/test_prroi_pooling2d.py): over integer-aligned ROIs of
    PH x PW whole cells the pooled output is the matching slice of F.avg_pool2d(feat, 2, 1)."""
    g = torch.Generator().manual_seed(2)
    feat = torch.rand(2, 4, 12, 12, generator=g, dtype=torch.float64)
    ph, pw = 5, 4
    rois = torch.tensor([[0, 0, 0, pw, ph], [1, 3, 2, 3 + pw, 2 + ph], [0, 7, 6, 7 + pw, 6 + ph]], dtype=torch.float64)
    out = prroi_pool_ref(feat, rois, ph, pw, 1.0)
    avg = F.avg_pool2d(feat, 2, 1)
    for k, (n, x, y) in enumerate(((0, 0, 0), (1, 3, 2), (0, 7, 6))):
        assert (out[k] - avg[n, :, y:y + ph, x:x + pw]).abs().max() < 1e-14


def test_degenerate_invalid_and_outside_rois_give_zeros():
    """(d) Zero outputs, zero box gradients and no contribution to the feature gradient."""
    N, C, H, W = 2, 2, 5, 7
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    adv, valid = adversarial_rois(N)
    outside = torch.tensor([[0, 20, 20, 25, 25], [1, -30, 1, -20, 4], [0, 1, 9, 3, 14]], dtype=torch.float32)
    rois = torch.cat([adv[[i for i, v in enumerate(valid) if not v]], outside]).double()
    gout = torch.randn(rois.shape[0], C, 3, 3, generator=g, dtype=torch.float64)
    out, gf, gr = gradients(feat, rois, 3, 3, 1.0, gout)
    assert torch.equal(out, torch.zeros_like(out))
    assert torch.equal(gr, torch.zeros_like(gr))
    assert torch.equal(gf, torch.zeros_like(gf))
    # and a valid ROI among them pools as it does alone
    mixed = torch.cat([rois[:3], torch.tensor([[1, 1.3, 0.7, 4.1, 3.9]], dtype=torch.float64), rois[3:]])
    alone = prroi_pool_ref(feat, mixed[3:4], 3, 3, 1.0)
    assert torch.equal(prroi_pool_ref(feat, mixed, 3, 3, 1.0)[3:4], alone) and alone.abs().max() > 0
    assert math.isfinite(float(alone.sum()))
