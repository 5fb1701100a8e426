"""PrRoIPool over ROI lists on the GPU (csrc/prroi.hip through mmtrack_amd.prroi_pool and the C entries): forward and
both gradients against tests/prroi_ref.py in float64, determinism, the reference's known-answer property, the
autograd contract, and a small IoU-style box refinement end to end.

Bars.  Forward: 1e-5 of the output maximum, the project's bar for this operator (tests/test_gpu_dimpnet.py).  The
gradients and the refined boxes: the same restatement evaluated in float32 on the CPU is compared with float64 over
every case below; 4 x its largest error, relative to the gradient maximum of its case (absolute, in pixels, for the
boxes), is the bar -- the factor 4 because the kernels sum in another order.  Both are printed.  Measured on an MI355X:

    box gradient      allowed 1.02e-05, largest 3.42e-06 of the case's maximum
    feature gradient  allowed 5.01e-06, largest 1.04e-06
    refined boxes     allowed 4.00e-05 px, measured 1.08e-05 px (boxes move up to 12.4 px)
"""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests.prroi_ref import NAN, INF, adversarial_rois, gradients, prroi_pool_ref

pytestmark = pytest.mark.gpu

N = 3
CHANNELS = (4, 8, 72, 256)            # a partly filled wave, several vectors per lane, more than one wave
MAPS = ((5, 7, 0.25), (12, 12, 0.0625))
POOLS = ((1, 1), (3, 3), (5, 5), (4, 4), (2, 5))
COUNTS = (0, 1, 11)
CASES = list(itertools.product(CHANNELS, range(len(MAPS)), POOLS))


def roi_list(H, W, scale, K):
    """K ROIs (image coordinates) on images 0 and 2 of 3 in shuffled order, image 1 empty: inside the map, across each
    border, fully outside, inside one cell, integer-aligned, one duplicate and two of the adversarial kind."""
    if K == 0:
        return torch.zeros(0, 5)
    cells = [[1.3, 0.7, W - 2.4, H - 1.6],
             [-1.7, 1.2, 2.3, 3.1], [1.1, -2.2, 3.6, 1.9], [W - 2.5, 0.4, W + 1.8, 2.7], [0.6, H - 1.9, 3.2, H + 2.3],
             [W + 3.0, H + 2.0, W + 6.0, H + 5.0], [2.2, 1.3, 2.7, 1.8], [1.0, 1.0, 4.0, 3.0],
             [1.3, 0.7, W - 2.4, H - 1.6], [1.0, 1.0, INF, 3.0], [1.0, 1.0, 3.0, 3.0]]
    index = [2.0, 0.0, 2.0, 0.0, 0.0, 2.0, 0.0, 2.0, 2.0, 0.0, NAN]
    rois = torch.tensor([[i] + [v / scale for v in c] for i, c in zip(index, cells)], dtype=torch.float32)
    if K == 1:
        return rois[:1].clone()
    return rois[torch.randperm(len(cells), generator=torch.Generator().manual_seed(7))][:K].clone()


def case_inputs(C, H, W, scale, ph, pw, K):
    g = torch.Generator().manual_seed(1000 * C + 10 * H + ph * 3 + pw + K)
    feat = torch.randn(N, C, H, W, generator=g)
    rois = roi_list(H, W, scale, K)
    gout = torch.randn(K, C, ph, pw, generator=g)
    return feat, rois, gout


def rel(a, b):
    m = float(b.abs().max())
    return float((a.double() - b).abs().max()) / m if m > 0 else float(a.abs().max())


@pytest.fixture(scope="module")
def reference():
    """Every case's float64 outputs and gradients, computed once, and the two gradient bars: 4 x the float32 CPU
    restatement's largest error against them."""
    ref, err_rois, err_feat = {}, 0.0, 0.0
    for (C, m, (ph, pw)), K in itertools.product(CASES, COUNTS):
        H, W, scale = MAPS[m]
        feat, rois, gout = case_inputs(C, H, W, scale, ph, pw, K)
        out, gf, gr = gradients(feat.double(), rois.double(), ph, pw, scale, gout.double())
        ref[(C, m, ph, pw, K)] = (out, gf, gr)
        if K:
            _, gf32, gr32 = gradients(feat, rois, ph, pw, scale, gout)
            err_rois, err_feat = max(err_rois, rel(gr32, gr)), max(err_feat, rel(gf32, gf))
    return ref, 4 * err_rois, 4 * err_feat


def run_op(feat, rois, ph, pw, scale, gout, channels_last):
    from mmtrack_amd.prroi_pool import prroi_pool2d
    f = feat.cuda()
    if channels_last:
        f = f.contiguous(memory_format=torch.channels_last)
    f.requires_grad_(True)
    r = rois.cuda().requires_grad_(True)
    out = prroi_pool2d(f, r, ph, pw, scale)
    out.backward(gout.cuda())
    return out.detach().cpu(), f.grad.cpu(), r.grad.cpu()


measured = {"rois": 0.0, "feat": 0.0}


@pytest.mark.parametrize("C,m,pool", CASES)
def test_forward_and_gradients_match_the_restatement(reference, C, m, pool):
    ref, bar_rois, bar_feat = reference
    (ph, pw), (H, W, scale) = pool, MAPS[m]
    for K in COUNTS:
        feat, rois, gout = case_inputs(C, H, W, scale, ph, pw, K)
        want, want_gf, want_gr = ref[(C, m, ph, pw, K)]
        out, gf, gr = run_op(feat, rois, ph, pw, scale, gout, channels_last=(C + K) % 2 == 0)
        assert out.shape == (K, C, ph, pw) and gf.shape == feat.shape and gr.shape == (K, 5)
        if K == 0:
            assert torch.equal(gf, torch.zeros_like(gf))
            continue
        e_out, e_gr, e_gf = rel(out, want), rel(gr, want_gr), rel(gf, want_gf)
        measured["rois"], measured["feat"] = max(measured["rois"], e_gr), max(measured["feat"], e_gf)
        print(f"C={C} {H}x{W} {ph}x{pw} K={K}: out {e_out:.2e} (1e-5)  grad_rois {e_gr:.2e} ({bar_rois:.2e})  "
              f"grad_feat {e_gf:.2e} ({bar_feat:.2e}); largest so far {measured['rois']:.2e} {measured['feat']:.2e}")
        assert e_out <= 1e-5
        assert e_gr <= bar_rois
        assert e_gf <= bar_feat
        assert torch.equal(gr[:, 0], torch.zeros(K))
        if K == 11:   # the ROIs that must give zeros: fully outside, an infinite coordinate, a NaN index
            dead = [k for k in range(K) if not torch.isfinite(rois[k]).all() or float(rois[k, 1]) * scale > W]
            assert len(dead) == 3
            for k in dead:
                assert torch.equal(out[k], torch.zeros(C, ph, pw)) and torch.equal(gr[k], torch.zeros(5))
            assert torch.equal(gf[1], torch.zeros(C, H, W))           # the image without ROIs


def test_adversarial_list_gives_zeros_and_the_restatement():
    """The list tests/test_prroi_host.py feeds the host build of the same arithmetic."""
    H, W, C, scale, ph, pw = 5, 7, 8, 0.5, 3, 3
    adv, valid = adversarial_rois(N)
    adv[:, 1:] /= scale
    g = torch.Generator().manual_seed(5)
    feat, gout = torch.randn(N, C, H, W, generator=g), torch.randn(adv.shape[0], C, ph, pw, generator=g)
    out, gf, gr = run_op(feat, adv, ph, pw, scale, gout, channels_last=True)
    want, want_gf, want_gr = gradients(feat.double(), adv.double(), ph, pw, scale, gout.double())
    for k, v in enumerate(valid):
        if not v:
            assert torch.equal(out[k], torch.zeros(C, ph, pw)) and torch.equal(gr[k], torch.zeros(5)), k
    assert torch.isfinite(out).all() and torch.isfinite(gf).all() and torch.isfinite(gr).all()
    assert rel(out, want) <= 1e-5
    _, gf32, gr32 = gradients(feat, adv, ph, pw, scale, gout)
    print(f"adversarial: grad_rois {rel(gr, want_gr):.2e} ({4 * rel(gr32, want_gr):.2e})  "
          f"grad_feat {rel(gf, want_gf):.2e} ({4 * rel(gf32, want_gf):.2e})")
    assert rel(gr, want_gr) <= 4 * rel(gr32, want_gr)
    assert rel(gf, want_gf) <= 4 * rel(gf32, want_gf)


def test_matches_the_one_roi_per_image_kernel():
    from mmtrack_amd import dimpnet
    from mmtrack_amd.prroi_pool import prroi_pool2d
    g = torch.Generator().manual_seed(9)
    feat = torch.randn(4, 72, 12, 12, generator=g).cuda()
    boxes = torch.tensor([[20.0, 30.0, 120.0, 150.0], [-40.0, 10.0, 60.0, 100.0], [150.0, 150.0, 260.0, 230.0],
                          [300.0, 300.0, 400.0, 400.0]])
    old = dimpnet.prroi_pool(feat, boxes, 1 / 16, 4, 4)
    rois = torch.cat([torch.arange(4.0)[:, None], boxes], 1).cuda()
    new = prroi_pool2d(feat, rois, 4, 4, 1 / 16)
    assert float((new - old).abs().max()) <= 1e-5 * float(old.abs().max())
    assert float(old.abs().max()) > 0.1


def test_bitwise_determinism_and_independence_of_other_images():
    C, (H, W, scale), (ph, pw) = 72, MAPS[1], (5, 5)
    feat, rois, gout = case_inputs(C, H, W, scale, ph, pw, 11)
    a = run_op(feat, rois, ph, pw, scale, gout, True)
    b = run_op(feat, rois, ph, pw, scale, gout, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # image 0's ROIs keep their places; the others (image 2 and the invalid ones) trade theirs in reverse
    on0 = rois[:, 0] == 0
    others = [k for k in range(11) if not on0[k]]
    perm = list(range(11))
    for k, src in zip(others, reversed(others)):
        perm[k] = src
    assert perm != list(range(11)) and int(on0.sum()) >= 3
    c = run_op(feat, rois[perm], ph, pw, scale, gout[perm], True)
    assert torch.equal(c[0], a[0][perm]) and torch.equal(c[2], a[2][perm])      # per ROI: out and the box gradient
    assert torch.equal(c[1][0], a[1][0]) and float(a[1][0].abs().max()) > 0     # image 0's feature gradient


def test_integer_aligned_rois_equal_avg_pool():
    from mmtrack_amd.prroi_pool import prroi_pool2d
    g = torch.Generator().manual_seed(2)
    feat = torch.rand(2, 16, 12, 12, generator=g).cuda()
    ph, pw = 7, 7
    rois = torch.tensor([[0, 0, 0, pw, ph], [1, 3, 2, 3 + pw, 2 + ph], [0, 4, 4, 4 + pw, 4 + ph]],
                        dtype=torch.float32).cuda()
    out = prroi_pool2d(feat, rois, ph, pw, 1.0)
    avg = F.avg_pool2d(feat, 2, 1)
    for k, (n, x, y) in enumerate(((0, 0, 0), (1, 3, 2), (0, 4, 4))):
        assert float((out[k] - avg[n, :, y:y + ph, x:x + pw]).abs().max()) <= 1e-5 * float(avg.abs().max())


def test_pitched_feature_map_through_the_c_entry():
    """A channel and column slice of a wider NHWC buffer is read in place and gives the bits of its packed copy."""
    from mmtrack_amd import _lib
    lib = _lib.load()
    H, W, C, Ww, Cw, scale, ph, pw, K = 12, 9, 8, 12, 24, 0.0625, 3, 3, 11
    g = torch.Generator().manual_seed(13)
    wide = torch.randn(N, H, Ww, Cw, generator=g).cuda()
    view = wide[:, :, 2:2 + W, 8:8 + C]
    packed = view.contiguous()
    rois = roi_list(H, W, scale, K).cuda()
    gout = torch.randn(K, C, ph, pw, generator=g).cuda()
    s = _lib.stream(wide.device)
    res = []
    for t in (view, packed):
        pitches = (t.stride(2), t.stride(1), t.stride(0))
        out = torch.full((K, C, ph, pw), NAN, device="cuda")
        gr = torch.full((K, 5), NAN, device="cuda")
        _lib.rc(lib.mmt_prroi_pool_rois(_lib.ptr(t), N, H, W, C, *pitches, _lib.ptr(rois), K, scale, ph, pw,
                                        _lib.ptr(out), s), "fwd")
        _lib.rc(lib.mmt_prroi_pool_rois_grad_rois(_lib.ptr(t), N, H, W, C, *pitches, _lib.ptr(rois), K, scale, ph, pw,
                                                  _lib.ptr(out), _lib.ptr(gout), _lib.ptr(gr), s), "grad_rois")
        res.append((out.cpu(), gr.cpu()))
    assert view.stride(2) == Cw and ctypes.c_void_p(view.data_ptr()).value != wide.data_ptr()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    want = prroi_pool_ref(packed.cpu().permute(0, 3, 1, 2).double(), rois.cpu().double(), ph, pw, scale)
    assert rel(res[0][0], want) <= 1e-5


def test_autograd_contract():
    from mmtrack_amd.prroi_pool import PrRoIPool2D, prroi_pool2d
    C, (H, W, scale), (ph, pw) = 8, MAPS[1], (3, 3)
    feat, rois, gout = case_inputs(C, H, W, scale, ph, pw, 11)
    a = run_op(feat, rois, ph, pw, scale, gout, channels_last=False)
    b = run_op(feat, rois, ph, pw, scale, gout, channels_last=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # grad_features comes back in the input's memory format
    for fmt in (torch.contiguous_format, torch.channels_last):
        f = feat.cuda().contiguous(memory_format=fmt).requires_grad_(True)
        prroi_pool2d(f, rois.cuda(), ph, pw, scale).backward(gout.cuda())
        assert f.grad.is_contiguous(memory_format=fmt)
    # only the required gradient is computed
    f, r = feat.cuda().requires_grad_(True), rois.cuda()
    prroi_pool2d(f, r, ph, pw, scale).backward(gout.cuda())
    assert r.grad is None and torch.equal(f.grad.cpu(), a[1])
    f, r = feat.cuda(), rois.cuda().requires_grad_(True)
    pool = PrRoIPool2D(ph, pw, scale)
    pool(f, r).backward(gout.cuda())
    assert f.grad is None and torch.equal(r.grad.cpu(), a[2]) and float(r.grad.abs().max()) > 0
    assert not prroi_pool2d(feat.cuda(), rois.cuda(), ph, pw, scale).requires_grad
    # the reference's assertion for a wrong dtype; an empty list without a launch
    with pytest.raises(AssertionError, match="Precise RoI Pooling only takes float input"):
        prroi_pool2d(feat.cuda().half(), rois.cuda(), ph, pw, scale)
    empty = prroi_pool2d(feat.cuda(), torch.zeros(0, 5, device="cuda"), ph, pw, scale)
    assert empty.shape == (0, C, ph, pw)
    with pytest.raises(ValueError):
        prroi_pool2d(feat.cuda()[:, :6], rois.cuda(), ph, pw, scale)     # C % 4


def _refine(pool, feats, weights, boxes, steps=5, step_length=1.0, decay=0.65):
    """A two-level IoU-style predictor (a 5 x 5 pool at 1/8, a 3 x 3 pool at 1/16, a fixed linear layer to one scalar
    per box) and gradient ascent on the boxes: step = step_length x gradient x box size, decaying per step."""
    boxes = boxes.clone()
    for _ in range(steps):
        b = boxes.clone().requires_grad_(True)
        p1, p2 = pool(feats[0], b, 5, 5, 1 / 8), pool(feats[1], b, 3, 3, 1 / 16)
        iou = (p1.flatten(1) * weights[0]).sum(1) + (p2.flatten(1) * weights[1]).sum(1)
        grad, = torch.autograd.grad(iou.sum(), b)
        size = torch.stack([b[:, 3] - b[:, 1], b[:, 4] - b[:, 2]], 1).detach().repeat(1, 2)
        boxes[:, 1:] = boxes[:, 1:] + step_length * grad[:, 1:] * size
        step_length *= decay
    return boxes


def test_box_refinement_end_to_end():
    from mmtrack_amd.prroi_pool import prroi_pool2d
    g = torch.Generator().manual_seed(21)
    feats = [torch.randn(2, 16, 12, 12, generator=g), torch.randn(2, 16, 6, 6, generator=g)]
    weights = [torch.randn(16 * 25, generator=g) / 20, torch.randn(16 * 9, generator=g) / 12]
    xy = torch.rand(12, 2, generator=g) * 50 + 5
    wh = torch.rand(12, 2, generator=g) * 30 + 12
    boxes = torch.cat([(torch.arange(12) % 2).float()[:, None], xy, xy + wh], 1)

    def ref(dt):
        return _refine(lambda f, b, ph, pw, s: prroi_pool_ref(f, b, ph, pw, s), [f.to(dt) for f in feats],
                       [w.to(dt) for w in weights], boxes.to(dt))
    want, cpu32 = ref(torch.float64), ref(torch.float32)
    bar = 4 * float((cpu32.double() - want).abs().max())
    got = _refine(prroi_pool2d, [f.cuda() for f in feats], [w.cuda() for w in weights], boxes.cuda()).cpu()
    err = float((got.double() - want).abs().max())
    moved = float((want - boxes.double()).abs().max())
    print(f"refined boxes: moved up to {moved:.3f} px; GPU vs float64 {err:.2e} px, allowed {bar:.2e} px")
    assert moved > 1.0
    assert torch.equal(got[:, 0], boxes[:, 0])
    assert err <= bar
