"""IoU-Net's predictor on the GPU (csrc/iounet.hip through mmtrack_amd.iounet and the C entries): the row-linear
kernel, predict_iou with its box gradient, the reference's ascent loop over predict_iou against the reference's own
run (tests/golden/iounet_det.npz), refine_boxes against that loop bit for bit, determinism and batch invariance, the
conv side (get_iou_feat, get_modulation), robustness to bad boxes and the module's contract.

Bars.  Head outputs follow tests/test_gpu_prroi.py: the restatement (tests/iounet_ref.py) evaluated in float32 on
the CPU is compared with float64 on the same inputs; 4 x its largest error over a group of cases is the group's bar --
relative to the case's maximum for IoU and gradient, absolute in pixels for boxes; the factor 4 because the kernels
sum in another order.  Conv outputs use the bars of tests/test_gpu_dimpnet.py: one conv within 1e-5 of its output
scale against float64 on the same operands, a chain within 1e-3.  The row-linear kernel: 1e-5 of the output scale.
Every bar and measured value is printed.  Measured on an MI355X:

    row-linear                  allowed 1e-5 of the output scale, largest 3.12e-07
    predict_iou, IoU            allowed 9.28e-06, largest 1.59e-06 of the case's maximum
    predict_iou, box gradient   allowed 5.33e-06, largest 1.54e-06
    golden ascent               boxes allowed 5.10e-04 px, measured 7.18e-05 px (boxes move up to 13.1 px);
                                returned IoU allowed 7.18e-06, measured 8.93e-07
    small-map ascents           boxes allowed 5.49e-04 px, largest 1.49e-04 px; IoU allowed 1.17e-05, largest 3.41e-06
    convs against the golden    f16x3 5.89e-07 (maps) / 2.48e-07 (modulation), fp32 7.10e-07 / 3.46e-07; allowed 1e-3
    one conv, small maps        f16x3 3.47e-07, fp32 7.15e-07; allowed 1e-5
"""
import functools
import os

import numpy as np
import pytest
import torch

from mmtrack_amd import _lib, synth
from tests.iounet_ref import (GOLDEN, HEADS, PREDICT_CASES, REFINE_B, REFINE_CASES, REFINE_ITERS, REFINE_P, SMALL_SIZE,
                              IoUNetRef, head_state_dict, inputs)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN, INF = float("nan"), float("inf")


def rel(a, b):
    m = float(b.abs().max())
    return float((a.double().cpu() - b).abs().max()) / m if m > 0 else float(a.abs().max())


def bits(*ts):
    return [t.detach().cpu().contiguous().view(torch.int32) for t in ts]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(bits(*a), bits(*b)))


@functools.lru_cache(maxsize=None)
def head_net(head, seed):
    from mmtrack_amd.iounet import AtomIoUNet
    return AtomIoUNet(head_state_dict(head, seed), device="cuda", precision="fp32")


@functools.lru_cache(maxsize=None)
def golden_net(precision):
    from mmtrack_amd.iounet import AtomIoUNet
    return AtomIoUNet(synth.make_iounet_state_dict(GOLDEN["seed"], input_dim=GOLDEN["input_dim"]), device="cuda",
                      precision=precision)


def case(head, seed, B, P, size=SMALL_SIZE):
    x = inputs(seed, B, P, size, pooled=HEADS[head]["pooled"])
    return x, [m.cuda() for m in x["mod"]], [f.cuda().contiguous(memory_format=torch.channels_last) for f in x["feat"]]


def gpu_iou_and_grad(net, mod, feat, boxes, gradient=None):
    bb = boxes.cuda().clone().requires_grad_(True)
    iou = net.predict_iou(mod, feat, bb)
    g = torch.ones_like(iou) if gradient is None else gradient.cuda()
    grad, = torch.autograd.grad(iou, bb, grad_outputs=g)
    return iou.detach(), grad


def reference_loop(net, mod, feat, init_boxes, iters, step_length, step_decay):
    """pytracking/tracker/dimp/dimp.py:727-752 (optimize_boxes_default) over net.predict_iou, for [B, P, 4] boxes
    -> (boxes after each step, the last outputs)."""
    output_boxes = init_boxes.cuda()
    if isinstance(step_length, (tuple, list)):
        step_length = torch.Tensor([step_length[0], step_length[0], step_length[1], step_length[1]]).cuda().view(1, 1, 4)
    trace = []
    for i_ in range(iters):
        bb_init = output_boxes.clone().detach()
        bb_init.requires_grad = True
        outputs = net.predict_iou(mod, feat, bb_init)
        outputs.backward(gradient=torch.ones_like(outputs))
        output_boxes = bb_init + step_length * bb_init.grad * bb_init[:, :, 2:].repeat(1, 1, 2)
        output_boxes.detach_()
        step_length *= step_decay
        trace.append(output_boxes)
    return torch.stack(trace), outputs.detach()


# ------------------------------------------------------------------------------------------------ 1. the row-linear
@pytest.mark.parametrize("Kd,N,bins", [(6400, 256, 25), (2304, 256, 9), (1800, 48, 25), (360, 80, 9)])
def test_row_linear_matches_float64(Kd, N, bins):
    """mmt_iounet_linear against float64 on the same operands: rows 1, 10, 17, 51 (a partial row tile, more than one,
    six modulation groups of 10 rows), with and without the modulation scale and the ReLU; 1e-5 of the output scale."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(Kd + N)
    W = torch.randn(N, Kd, generator=g) * (2.0 / Kd) ** 0.5
    b = torch.randn(N, generator=g) * 0.1
    Wd, bd = W.cuda(), b.cuda()
    worst = 0.0
    for R in (1, 10, 17, 51):
        X = torch.randn(R, Kd, generator=g)
        groups = (R + 9) // 10
        S = torch.rand(groups, Kd // bins, generator=g) + 0.25
        Xd, Sd = X.cuda(), S.cuda()
        need = lib.mmt_iounet_linear_ws_bytes(R, Kd, N)
        ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
        for scaled in (False, True):
            for relu in (False, True):
                Y = torch.full((R, N), NAN, dtype=torch.float32, device="cuda")
                rc = lib.mmt_iounet_linear(_lib.ptr(Xd), R, Kd, _lib.ptr(Wd), N, _lib.ptr(bd), _lib.ptr(Sd) if scaled else None,
                                           10, bins, int(relu), _lib.ptr(Y), _lib.ptr(ws), need, _lib.stream(Y.device))
                assert rc == 0
                x64 = X.double()
                if scaled:
                    x64 = x64 * S.double()[torch.arange(R) // 10].repeat_interleave(bins, dim=1)
                want = x64 @ W.double().T + b.double()
                scale = float(want.abs().max())
                if relu:
                    want = want.relu()
                err = float((Y.double().cpu() - want).abs().max()) / scale
                worst = max(worst, err)
                assert err <= 1e-5, (R, scaled, relu, err)
    print(f"row-linear Kd={Kd} N={N}: largest error {worst:.2e} of the output scale (allowed 1e-5)")


# ------------------------------------------------------------------------------------------------ 2. predict_iou
@pytest.fixture(scope="module")
def predict_reference():
    """Every PREDICT_CASES input's float64 IoU and box gradient, computed once, and the bars: 4 x the float32 CPU
    restatement's largest error.  Case ("real", 3, 10) runs with a non-trivial upstream gradient."""
    ref, e_iou, e_grad = {}, 0.0, 0.0
    for (head, B, P), seed in PREDICT_CASES.items():
        sd = head_state_dict(head, seed)
        x = inputs(seed, B, P, SMALL_SIZE, pooled=HEADS[head]["pooled"])
        up = upstream(head, B, P)
        iou, grad = IoUNetRef(sd).iou_and_grad(x["mod"], x["feat"], x["boxes"], up)
        iou32, grad32 = IoUNetRef(sd, dtype=torch.float32).iou_and_grad(x["mod"], x["feat"], x["boxes"], up)
        ref[(head, B, P)] = (iou, grad)
        e_iou, e_grad = max(e_iou, rel(iou32, iou)), max(e_grad, rel(grad32, grad))
    return ref, 4 * e_iou, 4 * e_grad


def upstream(head, B, P):
    if (head, B, P) != ("real", 3, 10):
        return None
    return torch.linspace(-1.0, 2.0, B * P).reshape(B, P)


@pytest.mark.parametrize("head,B,P", list(PREDICT_CASES))
def test_predict_iou_and_box_gradient_match_the_restatement(predict_reference, head, B, P):
    ref, bar_iou, bar_grad = predict_reference
    seed = PREDICT_CASES[(head, B, P)]
    x, mod, feat = case(head, seed, B, P)
    iou, grad = gpu_iou_and_grad(head_net(head, seed), mod, feat, x["boxes"], upstream(head, B, P))
    want_iou, want_grad = ref[(head, B, P)]
    assert iou.shape == (B, P) and grad.shape == (B, P, 4)
    e_iou, e_grad = rel(iou, want_iou), rel(grad, want_grad)
    print(f"{head} B={B} P={P}: iou {e_iou:.2e} (allowed {bar_iou:.2e})  box gradient {e_grad:.2e} (allowed {bar_grad:.2e})"
          f" of the case's maximum")
    assert float(want_grad.abs().max()) > 0
    assert e_iou <= bar_iou
    assert e_grad <= bar_grad


# ------------------------------------------------------------------------------------------------ 3. / 4. the ascent
@pytest.fixture(scope="module")
def golden():
    """The golden, its inputs, the golden's modulation and maps on the GPU (rounded to float32, what the head takes),
    and the box / IoU bars of the full-size ascent: 4 x the error of the restatement run in float32 on the CPU, on
    those float32 inputs, against the reference's float64 run."""
    g = np.load(os.path.join(HERE, "golden", "iounet_det.npz"))
    sd = synth.make_iounet_state_dict(GOLDEN["seed"], input_dim=GOLDEN["input_dim"])
    x = inputs(GOLDEN["seed"], GOLDEN["B"], GOLDEN["P"], GOLDEN["size"], input_dim=GOLDEN["input_dim"])
    ref64 = IoUNetRef(sd)
    with torch.no_grad():
        mod = [m.float() for m in ref64.get_modulation(x["back"], x["bb"])]
        feat = [f.float() for f in ref64.get_iou_feat(x["back"])]
    assert rel(mod[0], torch.from_numpy(g["mod3"])) < 1e-6 and rel(feat[0][:, ::16], torch.from_numpy(g["feat3_ch"])) < 1e-6
    steps32, iou32 = IoUNetRef(sd, dtype=torch.float32).refine(mod, feat, x["boxes"], GOLDEN["iters"])
    bar_px = 4 * float((steps32.double() - torch.from_numpy(g["boxes_steps"])).abs().max())
    bar_iou = 4 * rel(iou32, torch.from_numpy(g["iou_final"]))
    dev = ([m.cuda() for m in mod], [f.cuda().contiguous(memory_format=torch.channels_last) for f in feat])
    return g, x, dev, (bar_px, bar_iou)


def test_reference_loop_over_predict_iou_reproduces_the_golden(golden):
    """The reference's optimize_boxes_default, written here as it is there, over predict_iou: 5 steps on the golden
    inputs (real head, B = 2, P = 10, maps 36 x 36 and 18 x 18); the boxes after each step and the returned IoU
    against the reference's own run (tests/golden/iounet_det.npz), within the derived bars."""
    g, x, (mod, feat), (bar_px, bar_iou) = golden
    net = golden_net("fp32")
    steps, iou = reference_loop(net, mod, feat, x["boxes"], GOLDEN["iters"], 1.0, 1.0)
    want = torch.from_numpy(g["boxes_steps"])
    e_px = float((steps.double().cpu() - want).abs().max())
    e_iou = rel(iou, torch.from_numpy(g["iou_final"]))
    moved = float((want[-1] - x["boxes"].double()).abs().max())
    print(f"golden ascent: boxes {e_px:.2e} px (allowed {bar_px:.2e}), iou {e_iou:.2e} (allowed {bar_iou:.2e}); boxes "
          f"move up to {moved:.1f} px")
    assert e_px <= bar_px and e_iou <= bar_iou


def test_refine_boxes_equals_the_loop_bitwise_on_the_golden(golden):
    """refine_boxes runs the kernels predict_iou and its backward run, so it gives the loop's bits; the IoU it returns
    is that of the boxes before the last update."""
    _, x, (mod, feat), _ = golden
    net = golden_net("fp32")
    steps, iou = reference_loop(net, mod, feat, x["boxes"], GOLDEN["iters"], 1.0, 1.0)
    boxes, riou = net.refine_boxes(mod, feat, x["boxes"].cuda(), GOLDEN["iters"], 1.0, 1.0)
    assert same_bits((boxes, riou), (steps[-1], iou))
    assert same_bits((riou,), (net.predict_iou(mod, feat, steps[-2]),))
    assert not torch.equal(riou, net.predict_iou(mod, feat, steps[-1]))


@pytest.fixture(scope="module")
def refine_reference():
    ref, e_px, e_iou = {}, 0.0, 0.0
    for (head, step, decay), seed in REFINE_CASES.items():
        sd = head_state_dict(head, seed)
        x = inputs(seed, REFINE_B, REFINE_P, SMALL_SIZE, pooled=HEADS[head]["pooled"])
        s64, i64 = IoUNetRef(sd).refine(x["mod"], x["feat"], x["boxes"], REFINE_ITERS, step, decay)
        s32, i32 = IoUNetRef(sd, dtype=torch.float32).refine(x["mod"], x["feat"], x["boxes"], REFINE_ITERS, step, decay)
        ref[(head, step, decay)] = (s64, i64)
        e_px, e_iou = max(e_px, float((s32.double() - s64).abs().max())), max(e_iou, rel(i32, i64))
    return ref, 4 * e_px, 4 * e_iou


@pytest.mark.parametrize("head,step,decay", list(REFINE_CASES))
def test_refine_boxes_scalar_and_pair_steps_with_decay(refine_reference, head, step, decay):
    """refine_boxes with a scalar and a (position, size) step and step_decay 0.5, both heads: the bits of the loop
    over predict_iou, the float64 restatement within the derived bars, and the IoU of the pre-last-update boxes."""
    ref, bar_px, bar_iou = refine_reference
    seed = REFINE_CASES[(head, step, decay)]
    x, mod, feat = case(head, seed, REFINE_B, REFINE_P)
    net = head_net(head, seed)
    boxes, iou = net.refine_boxes(mod, feat, x["boxes"].cuda(), REFINE_ITERS, step, decay)
    steps, liou = reference_loop(net, mod, feat, x["boxes"], REFINE_ITERS, step, decay)
    assert same_bits((boxes, iou), (steps[-1], liou))
    assert same_bits((iou,), (net.predict_iou(mod, feat, steps[-2]),))
    s64, i64 = ref[(head, step, decay)]
    e_px, e_iou = float((boxes.double().cpu() - s64[-1]).abs().max()), rel(iou, i64)
    print(f"{head} step={step} decay={decay}: boxes {e_px:.2e} px (allowed {bar_px:.2e}), iou {e_iou:.2e} (allowed "
          f"{bar_iou:.2e}); boxes move up to {float((s64[-1] - x['boxes'].double()).abs().max()):.1f} px")
    assert e_px <= bar_px and e_iou <= bar_iou
    # decay 0.5 on a scalar step as well
    if not isinstance(step, tuple):
        b2, i2 = net.refine_boxes(mod, feat, x["boxes"].cuda(), REFINE_ITERS, step, 0.5)
        s2, l2 = reference_loop(net, mod, feat, x["boxes"], REFINE_ITERS, step, 0.5)
        assert same_bits((b2, i2), (s2[-1], l2)) and not torch.equal(b2, boxes)


# ------------------------------------------------------------------------------------------------ 5. bits
@pytest.mark.parametrize("head", ["real", "small"])
def test_determinism_and_batch_invariance_bitwise(head):
    seed = 11
    net = head_net(head, seed)
    x, mod, feat = case(head, seed, 3, 10)
    b0 = x["boxes"].cuda()
    run = lambda m, f, b: net.refine_boxes(m, f, b, 3, 0.2, 1.0) + gpu_iou_and_grad(net, m, f, b)   # noqa: E731
    full = run(mod, feat, b0)
    assert same_bits(full, run(mod, feat, b0))                                   # two runs
    for b in range(3):                                                            # a sequence alone
        one = run([m[b:b + 1] for m in mod], [f[b:b + 1] for f in feat], b0[b:b + 1])
        assert same_bits(one, [t[b:b + 1] for t in full]), b
    few = run(mod, feat, b0[:, :4].contiguous())                                  # 4 of the 10 proposals
    assert same_bits(few, [t[:, :4] for t in full])


def test_320_rows_equal_their_per_sequence_calls_bitwise():
    """B = 32, P = 10 (320 rows: 20 row tiles) on the small maps, real head: sequences 0 and 31 of the one call equal
    their own calls."""
    seed = 12
    net = head_net("real", seed)
    x, mod, feat = case("real", seed, 32, 10)
    b0 = x["boxes"].cuda()
    full = net.refine_boxes(mod, feat, b0, 3, 0.2, 1.0)
    assert same_bits(full, net.refine_boxes(mod, feat, b0, 3, 0.2, 1.0))
    for b in (0, 31):
        one = net.refine_boxes([m[b:b + 1] for m in mod], [f[b:b + 1] for f in feat], b0[b:b + 1], 3, 0.2, 1.0)
        assert same_bits(one, [t[b:b + 1] for t in full]), b


# ------------------------------------------------------------------------------------------------ 6. the conv side
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_iou_feat_and_modulation_match_the_golden(golden, precision):
    """get_iou_feat (two-conv chains) and get_modulation (conv, pool, linears) at DeT's input dims, B = 2, full-size
    maps, against the reference's float64 run: 1e-3 of each output's scale, the project's bar for a chain."""
    g, x, _, _ = golden
    net = golden_net(precision)
    back = [t.cuda() for t in x["back"]]
    f3, f4 = net.get_iou_feat(back)
    m3, m4 = net.get_modulation(back, x["bb"].cuda())
    assert f3.shape == (2, 256, 36, 36) and f4.shape == (2, 256, 18, 18) and m3.shape == m4.shape == (2, 256, 1, 1)
    assert f3.is_contiguous(memory_format=torch.channels_last)
    errs = dict(feat3=rel(f3[:, ::16], torch.from_numpy(g["feat3_ch"])), feat4=rel(f4[:, ::16], torch.from_numpy(g["feat4_ch"])),
                mod3=rel(m3, torch.from_numpy(g["mod3"])), mod4=rel(m4, torch.from_numpy(g["mod4"])))
    print(precision, {k: f"{v:.2e}" for k, v in errs.items()}, "(allowed 1e-3 of scale)")
    assert max(errs.values()) <= 1e-3
    # a bound of max|feat| instead of the computed range gives the same maps at a coarser or equal input scale
    if precision == "f16x3":
        bound = [float(t.abs().max()) for t in back]
        g3, g4 = net.get_iou_feat(back, feat_max=bound)
        assert torch.equal(g3, f3) and torch.equal(g4, f4)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_conv_side_matches_the_restatement_on_small_maps(precision):
    """The same on 12 x 12 / 6 x 6 maps against the restatement in float64 (other shapes than the golden's): a single
    conv within 1e-5 of its output scale, the chains and the modulation within 1e-3."""
    net = golden_net(precision)
    x = inputs(21, 2, 1, SMALL_SIZE, input_dim=GOLDEN["input_dim"])
    ref = IoUNetRef(synth.make_iounet_state_dict(GOLDEN["seed"], input_dim=GOLDEN["input_dim"]))
    with torch.no_grad():
        want_feat = ref.get_iou_feat(x["back"])
        want_mod = ref.get_modulation(x["back"], x["bb"])
        want_one = ref._conv(x["back"][0].double(), "conv3_1t", 1)
    back = [t.cuda() for t in x["back"]]
    one = net._chain("conv3_1t", None, back[0], None).permute(0, 3, 1, 2)
    feat = net.get_iou_feat(back)
    mod = net.get_modulation(back, x["bb"].cuda())
    e_one = rel(one, want_one)
    e_chain = max(rel(a, b) for a, b in zip(feat, want_feat))
    e_mod = max(rel(a, b) for a, b in zip(mod, want_mod))
    print(f"{precision}: one conv {e_one:.2e} (allowed 1e-5), chains {e_chain:.2e}, modulation {e_mod:.2e} (allowed 1e-3)")
    assert e_one <= 1e-5 and e_chain <= 1e-3 and e_mod <= 1e-3


def test_modulation_layouts_give_the_same_iou():
    seed = PREDICT_CASES[("real", 3, 10)]
    net = head_net("real", seed)
    x, mod, feat = case("real", seed, 3, 10)
    b = x["boxes"].cuda()
    base = net.predict_iou(mod, feat, b)
    assert torch.equal(base, net.predict_iou([m.reshape(3, -1, 1, 1) for m in mod], feat, b))
    mean = [m.mean(0) for m in mod]                                   # what the tracker stores
    expanded = net.predict_iou([m[None].expand(3, -1).contiguous() for m in mean], feat, b)
    for single in (mean, [m[None] for m in mean], [m.reshape(1, -1, 1, 1) for m in mean]):
        assert torch.equal(expanded, net.predict_iou(single, feat, b))
    assert not torch.equal(expanded, base)
    with pytest.raises(ValueError):
        net.predict_iou([m[:2] for m in mod], feat, b)


# ------------------------------------------------------------------------------------------------ 7. robustness
def test_bad_boxes_leave_the_valid_ones_alone():
    """A proposal list holding a NaN box, a box of negative size and a box fully outside the image (ordinary inputs
    that pool to zeros): the valid boxes' IoU, gradient and refined boxes are bit-equal to a call without the bad
    ones, the bad boxes' IoUs are finite where the box is finite (the head applied to zeros), their gradients zero."""
    seed = PREDICT_CASES[("small", 1, 10)]
    net = head_net("small", seed)
    x, mod, feat = case("small", seed, 1, 10)
    good = x["boxes"].cuda()
    bad = torch.tensor([[[NAN, 20.0, 30.0, 30.0], [40.0, 40.0, -12.0, 20.0], [400.0, 300.0, 25.0, 25.0],
                         [20.0, 20.0, INF, 10.0]]], device="cuda")
    mixed = torch.cat([good[:, :3], bad[:, :2], good[:, 3:], bad[:, 2:]], dim=1)
    keep = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11]
    iou, grad = gpu_iou_and_grad(net, mod, feat, mixed)
    want = gpu_iou_and_grad(net, mod, feat, good)
    assert same_bits((iou[:, keep], grad[:, keep]), want)
    zero_iou = net.predict_iou(mod, [torch.zeros_like(f) for f in feat], good[:, :1])
    for i in (3, 4, 12, 13):
        assert torch.equal(grad[0, i], torch.zeros(4, device="cuda")), i
        assert torch.equal(iou[0, i], zero_iou[0, 0]) and bool(torch.isfinite(iou[0, i])), i
    rb, ri = net.refine_boxes(mod, feat, mixed, 3, 0.2, 1.0)
    wb, wi = net.refine_boxes(mod, feat, good, 3, 0.2, 1.0)
    assert same_bits((rb[:, keep], ri[:, keep]), (wb, wi))
    assert bool(torch.isfinite(ri[0, [4, 12]]).all()) and torch.equal(rb[0, 4], mixed[0, 4]) and torch.equal(rb[0, 12], mixed[0, 12])


# ------------------------------------------------------------------------------------------------ 8. the contract
def test_contract_empty_layouts_and_streams():
    seed = PREDICT_CASES[("small", 3, 10)]
    net = head_net("small", seed)
    x, mod, feat = case("small", seed, 3, 10)
    b = x["boxes"].cuda()
    want = gpu_iou_and_grad(net, mod, feat, b)
    # no proposals: empty tensors, no launch, a zero-size gradient
    e = b[:, :0].clone().requires_grad_(True)
    iou = net.predict_iou(mod, feat, e)
    assert iou.shape == (3, 0)
    iou.sum().backward()
    assert e.grad.shape == (3, 0, 4)
    rb, ri = net.refine_boxes(mod, feat, b[:, :0])
    assert rb.shape == (3, 0, 4) and ri.shape == (3, 0)
    # NCHW-contiguous and non-contiguous maps are converted once; non-contiguous boxes and modulation likewise
    nchw = [f.contiguous() for f in feat]
    assert same_bits(gpu_iou_and_grad(net, mod, nchw, b), want)
    wide = [torch.cat([f, f], dim=3)[..., :f.shape[3]] for f in nchw]
    assert not wide[0].is_contiguous()
    assert same_bits(gpu_iou_and_grad(net, mod, wide, b), want)
    sliced = [torch.cat([f, f], dim=1).contiguous(memory_format=torch.channels_last)[:, :f.shape[1]] for f in feat]
    assert same_bits(gpu_iou_and_grad(net, mod, sliced, b), want)   # a channel slice of a wider map: read in place
    bt = torch.cat([b, b], dim=2)[..., :4]
    assert same_bits(gpu_iou_and_grad(net, [torch.cat([m, m], 1)[:, :m.shape[1]] for m in mod], feat, bt), want)
    # gradients go to the proposals only
    f_req = [f.clone().requires_grad_(True) for f in feat]
    m_req = [m.clone().requires_grad_(True) for m in mod]
    bb = b.clone().requires_grad_(True)
    net.predict_iou(m_req, f_req, bb).sum().backward()
    assert bb.grad is not None and all(t.grad is None for t in f_req + m_req)
    with pytest.raises(ValueError):
        net.predict_iou(mod, feat, b.double())
    # a non-default current stream
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = gpu_iou_and_grad(net, mod, feat, b)
        rs = net.refine_boxes(mod, feat, b, 3, 0.2, 1.0)
    s.synchronize()
    assert same_bits(got, want) and same_bits(rs, net.refine_boxes(mod, feat, b, 3, 0.2, 1.0))
