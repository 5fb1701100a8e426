"""IoU-Net's predictor (the reference's ``AtomIoUNet``, ltr/models/bbreg/atom_iou_net.py) on the HIP kernels of
csrc/iounet.hip, csrc/prroi.hip and the conv entry points.

``AtomIoUNet(state_dict)`` keeps the reference module's inference contract:

* ``get_iou_feat([feat3, feat4])``         conv3_1t -> conv3_2t and conv4_1t -> conv4_2t (3 x 3, bias, BN, ReLU);
* ``get_modulation([feat3, feat4], bb)``   conv3_1r / conv4_1r, PrRoIPool 3 x 3 at 1/8 and 1 x 1 at 1/16 of the target
  box, fc3_1r, fc34_3r / fc34_4r -> two ``[B, C, 1, 1]`` modulation vectors;
* ``predict_iou(modulation, feat, proposals)``  ``[B, P, 4]`` xywh boxes -> ``[B, P]``, differentiable in ``proposals``
  (and only in them), so the reference's own ``optimize_boxes_default`` / ``optimize_boxes_relative`` loops
  (``bb_init.requires_grad = True; outputs.backward(gradient=ones)``) run on it unchanged;
* ``refine_boxes(modulation, feat, init_boxes, iters, step_length, step_decay)``  that loop in one library call
  (mmt_iounet_refine), giving the same bits as the loop over ``predict_iou``.

Dimensions are read from the weight shapes (the plain dimp50's input_dim (128, 256) and DeT's (512, 1024) both load).
BatchNorm (eval, eps 1e-5) is folded into each conv and linear in float64 on the host.  The head is fp32 throughout
whatever ``precision`` says; ``precision`` ("f16x3", default, or "fp32") selects the conv kernels as in ``DiMPNet``.
There is no CPU path: CPU tensors raise NotImplementedError and a missing libmmtrack.so is an ImportError.  No torch
matmul or conv runs on the GPU; launches are ordered on torch's current stream.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .dimpnet import MAX_WORDS, _Conv, range_scale
from .prroi_pool import _channels_last

__all__ = ["AtomIoUNet"]

_rc, _p, _stream = _lib.rc, _lib.ptr, _lib.stream
POOL3, POOL4 = 5, 3                 # PrRoIPool2D(5, 5, 1/8) and (3, 3, 1/16) of the proposals
SCALE3, SCALE4 = 1 / 8, 1 / 16


def _fold_bn(w, b, bn):
    """Linear / flattened conv weight [N, K] and bias with eval BatchNorm folded in, float64 -> float32."""
    g, beta, mean, var = (t.detach().double() for t in bn)
    s = g / torch.sqrt(var + 1e-5)
    return (w.detach().double() * s[:, None]).float().contiguous(), ((b.detach().double() - mean) * s + beta).float()


class _PredictIoU(torch.autograd.Function):
    """predict_iou as an autograd node of ``proposals``: backward runs the forward again with the upstream
    gradient, because the masked hidden gradient is a by-product of the head's reduce step."""

    @staticmethod
    def forward(ctx, proposals, net, mods, feats):
        ctx.net, ctx.mods, ctx.feats = net, mods, feats
        ctx.save_for_backward(proposals)
        return net._predict(mods, feats, proposals.detach(), None, False)[0]

    @staticmethod
    def backward(ctx, grad_iou):
        proposals, = ctx.saved_tensors
        grad = ctx.net._predict(ctx.mods, ctx.feats, proposals.detach(), grad_iou.contiguous().float(), True)[1]
        return grad, None, None, None


class AtomIoUNet:
    def __init__(self, state_dict, prefix="bb_regressor.", device=None, precision="f16x3"):
        if precision not in ("f16x3", "fp32"):
            raise ValueError(f"precision must be 'f16x3' or 'fp32', got {precision!r}")
        self.precision = precision
        self.dev = torch.device(device if device is not None else "cuda")
        if self.dev.type == "cuda" and self.dev.index is None and torch.cuda.is_available():
            self.dev = torch.device("cuda", torch.cuda.current_device())
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        if "iou_predictor.weight" not in sd:
            raise ValueError(f"no {prefix}iou_predictor.weight in the state dict")

        def bn(pre):
            return tuple(sd[f"{pre}.{t}"] for t in ("weight", "bias", "running_mean", "running_var"))

        w3, w4 = sd["fc3_rt.linear.weight"], sd["fc4_rt.linear.weight"]
        self.c3, self.c4 = sd["conv3_2t.0.weight"].shape[0], sd["conv4_2t.0.weight"].shape[0]
        self.n3, self.n4 = w3.shape[0], w4.shape[0]
        self.input_dim = (sd["conv3_1t.0.weight"].shape[1], sd["conv4_1t.0.weight"].shape[1])
        if w3.shape[1] != self.c3 * POOL3 * POOL3 or w4.shape[1] != self.c4 * POOL4 * POOL4:
            raise ValueError("fc3_rt / fc4_rt do not take 5 x 5 / 3 x 3 bins of conv3_2t / conv4_2t's channels")
        if self.c3 % 4 or self.c4 % 4:
            raise ValueError(f"pooled channels must be multiples of 4, got {(self.c3, self.c4)}")
        if self.n3 % 16 or self.n4 % 16:
            raise ValueError(f"hidden widths must be multiples of 16, got {(self.n3, self.n4)}")
        if tuple(sd["iou_predictor.weight"].shape) != (1, self.n3 + self.n4):
            raise ValueError("iou_predictor.weight does not take the two hidden layers")
        to = lambda t: t.to(self.dev)   # noqa: E731
        self.w3, self.b3 = (to(t) for t in _fold_bn(w3, sd["fc3_rt.linear.bias"], bn("fc3_rt.bn")))
        self.w4, self.b4 = (to(t) for t in _fold_bn(w4, sd["fc4_rt.linear.bias"], bn("fc4_rt.bn")))
        self.wp = to(sd["iou_predictor.weight"].detach().float().reshape(-1).contiguous())
        self.bp = float(sd["iou_predictor.bias"].detach().float().reshape(-1)[0])
        # the modulation side's small layers as linears: a 3 x 3 conv on a 3 x 3 map, and 1 x 1 convs on 1 x 1 maps
        self.lin_r = {}
        for name in ("fc3_1r", "fc34_3r", "fc34_4r"):
            w = sd[f"{name}.0.weight"]
            wf, bf = _fold_bn(w.reshape(w.shape[0], -1), sd[f"{name}.0.bias"], bn(f"{name}.1"))
            self.lin_r[name] = (to(wf), to(bf))
        f16 = precision == "f16x3"
        self.convs = {}
        for name in ("conv3_1r", "conv3_1t", "conv3_2t", "conv4_1r", "conv4_1t", "conv4_2t"):
            w = sd[f"{name}.0.weight"]
            ok = w.shape[0] % 64 == 0 and w.shape[1] % 32 == 0   # what the conv entry points take
            self.convs[name] = _Conv(w, bn=bn(f"{name}.1"), bias=sd[f"{name}.0.bias"], stride=1, pad=1, dev=self.dev,
                                     f16x3=f16) if ok else None
        self._bufs = {}

    # ------------------------------------------------------------------------------------------------ helpers
    def _cuda(self, *tensors):
        for t in tensors:
            if not t.is_cuda:
                raise NotImplementedError("AtomIoUNet only supports GPU (cuda) tensors; there is no CPU path")

    def _buf(self, name, n):
        b = self._bufs.get(name)
        if b is None or b.numel() < n:
            b = self._bufs[name] = torch.empty(n, dtype=torch.float32, device=self.dev)
        return b[:n]

    def _ws(self, nbytes):
        return self._buf("ws", (nbytes + 3) // 4)

    def _conv(self, name, x, N, H, W, relu=True, **kw):
        conv = self.convs[name]
        if conv is None:
            raise ValueError(f"{name}: the conv kernels take output channels % 64 == 0 and input channels % 32 == 0")
        out = torch.empty(N, H, W, conv.cout, dtype=torch.float32, device=x.device)
        conv(_lib.load(), x, N, H, W, out, _stream(x.device), relu=relu, ws=self._ws, **kw)
        return out

    def _chain(self, first, second, x, feat_max):
        """second(first(x)) on an NCHW (or channels_last) map -> NHWC.  f16x3: the first conv's input scale comes
        from feat_max (a bound of max|x|) or, without it, from the tensor (one device-to-host sync); the second conv
        reads the max words the first accumulated."""
        N, _, H, W = x.shape
        xn = x.detach().float().permute(0, 2, 3, 1).contiguous()
        if self.precision != "f16x3":
            y = self._conv(first, xn, N, H, W)
            return self._conv(second, y, N, H, W) if second else y
        m = float(feat_max) if feat_max is not None else float(xn.abs().max())
        if not second:
            return self._conv(first, xn, N, H, W, x_scale=range_scale(m))
        words = torch.zeros(MAX_WORDS, dtype=torch.float32, device=x.device)
        y = self._conv(first, xn, N, H, W, x_scale=range_scale(m), y_max=words)
        return self._conv(second, y, N, H, W, x_max=words)

    def _linear(self, x, wb, relu=True):
        """act(x [R, Kd] . w [N, Kd]^T + b) through mmt_iounet_linear."""
        w, b = wb
        lib = _lib.load()
        R, Kd = x.shape
        N = w.shape[0]
        x = x.contiguous()
        y = torch.empty(R, N, dtype=torch.float32, device=x.device)
        need = lib.mmt_iounet_linear_ws_bytes(R, Kd, N)
        _rc(lib.mmt_iounet_linear(_p(x), R, Kd, _p(w), N, _p(b), None, 1, 1, 1 if relu else 0, _p(y), _p(self._ws(need)),
                                  need, _stream(x.device)), "mmt_iounet_linear")
        return y

    @staticmethod
    def _feat_max(feat_max, i):
        return None if feat_max is None else (feat_max[i] if isinstance(feat_max, (tuple, list)) else feat_max)

    # ------------------------------------------------------------------------------------------------ the contract
    def get_iou_feat(self, feat2, feat_max=None):
        """[feat3, feat4] backbone maps ``[B, C, H, W]`` (5-dimensional inputs are flattened as the reference does)
        -> the two IoU feature maps ``[B, C, H, W]``, channels last in memory, which predict_iou reads in place.
        f16x3: ``feat_max`` (a number, or one per level) bounds max|feat|; without it the range is computed from
        each tensor, which synchronises with the device once per level."""
        feat2 = [f.reshape(-1, *f.shape[-3:]) if f.dim() == 5 else f for f in feat2]
        self._cuda(*feat2)
        with torch.cuda.device(feat2[0].device):
            c3 = self._chain("conv3_1t", "conv3_2t", feat2[0], self._feat_max(feat_max, 0))
            c4 = self._chain("conv4_1t", "conv4_2t", feat2[1], self._feat_max(feat_max, 1))
        return c3.permute(0, 3, 1, 2), c4.permute(0, 3, 1, 2)

    def get_modulation(self, feat, bb, feat_max=None):
        """[feat3, feat4] backbone maps of the reference images and their target boxes ``bb [B, 4]`` (xywh, image
        coordinates) -> the modulation vectors (``[B, C3, 1, 1]``, ``[B, C4, 1, 1]``).  ``feat_max`` as in
        get_iou_feat."""
        f3, f4 = feat
        self._cuda(f3, f4, bb)
        lib = _lib.load()
        B = bb.shape[0]
        with torch.cuda.device(f3.device):
            s = _stream(f3.device)
            c3 = self._chain("conv3_1r", None, f3, self._feat_max(feat_max, 0))
            c4 = self._chain("conv4_1r", None, f4, self._feat_max(feat_max, 1))
            b = bb.detach().float().reshape(B, 4)
            rois = torch.cat([torch.arange(B, dtype=torch.float32, device=b.device)[:, None], b[:, :2],
                              b[:, :2] + b[:, 2:]], dim=1).contiguous()
            pooled = []
            for c, bins, scale in ((c3, 3, SCALE3), (c4, 1, SCALE4)):
                n, h, w, ch = c.shape
                out = torch.empty(B, ch * bins * bins, dtype=torch.float32, device=c.device)
                _rc(lib.mmt_prroi_pool_rois(_p(c), n, h, w, ch, ch, w * ch, h * w * ch, _p(rois), B, scale, bins, bins,
                                            _p(out), s), "mmt_prroi_pool_rois")
                pooled.append(out)
            both = torch.cat([self._linear(pooled[0], self.lin_r["fc3_1r"]), pooled[1]], dim=1)
            m3 = self._linear(both, self.lin_r["fc34_3r"])
            m4 = self._linear(both, self.lin_r["fc34_4r"])
        return m3.reshape(B, -1, 1, 1), m4.reshape(B, -1, 1, 1)

    def _modulation(self, m, B, C):
        """[B, C], [B, C, 1, 1] or one vector (the tracker stores mean(0)) -> contiguous float32 [B, C]."""
        if m.numel() == C:
            return m.detach().float().reshape(1, C).expand(B, C).contiguous()
        if m.numel() != B * C:
            raise ValueError(f"modulation of {tuple(m.shape)} for {B} sequences of {C} channels")
        return m.detach().float().reshape(B, C).contiguous()

    def _args(self, modulation, feat, boxes):
        """The library's arguments for boxes [B, P, 4]: head, maps, modulation; and the tensors they point into."""
        f3, f4 = feat
        self._cuda(f3, f4, boxes, *modulation)
        if boxes.dim() != 3 or boxes.shape[2] != 4 or f3.dim() != 4 or f4.dim() != 4:
            raise ValueError(f"proposals must be [B, P, 4] and the maps [B, C, H, W], got {tuple(boxes.shape)}, "
                             f"{tuple(f3.shape)}, {tuple(f4.shape)}")
        B, P = boxes.shape[:2]
        if f3.shape[0] != B or f4.shape[0] != B or f3.shape[1] != self.c3 or f4.shape[1] != self.c4:
            raise ValueError(f"maps of {tuple(f3.shape)}, {tuple(f4.shape)} for {B} sequences of {(self.c3, self.c4)} "
                             f"channels")
        keep = [self._modulation(modulation[0], B, self.c3), self._modulation(modulation[1], B, self.c4)]
        maps = []
        for f in (f3, f4):
            t, (pix, row, img) = _channels_last(f.detach().float())
            keep.append(t)
            maps.append(_lib.MmtIounetMap(t.data_ptr(), f.shape[2], f.shape[3], pix, row, img))
        head = _lib.MmtIounetHead(self.w3.data_ptr(), self.b3.data_ptr(), self.w4.data_ptr(), self.b4.data_ptr(),
                                  self.wp.data_ptr(), self.bp, self.c3, self.c4, self.n3, self.n4)
        fa = _lib.MmtIounetFeat(B, 0, maps[0], maps[1])
        need = _lib.load().mmt_iounet_ws_bytes(B * P, self.c3 * POOL3 * POOL3, self.c4 * POOL4 * POOL4, self.n3,
                                                self.n4)
        return head, fa, keep, need

    def _predict(self, modulation, feat, boxes, grad_iou, want_grad):
        B, P = boxes.shape[:2]
        iou = torch.empty(B, P, dtype=torch.float32, device=boxes.device)
        grad = torch.zeros(B, P, 4, dtype=torch.float32, device=boxes.device) if want_grad else None
        if B * P == 0:
            self._cuda(boxes)
            return iou, grad
        head, fa, keep, need = self._args(modulation, feat, boxes)
        bx = boxes.float().contiguous()
        with torch.cuda.device(boxes.device):
            _rc(_lib.load().mmt_iounet_predict(ctypes.byref(head), ctypes.byref(fa), _p(keep[0]), _p(keep[1]), _p(bx), P,
                                               _p(grad_iou), _p(iou), _p(grad), _p(self._ws(need)), need,
                                               _stream(boxes.device)), "mmt_iounet_predict")
        return iou, grad

    def predict_iou(self, modulation, feat, proposals):
        """IoU of ``proposals [B, P, 4]`` (xywh, image coordinates) -> ``[B, P]``.  ``modulation``: the two vectors
        as ``[B, C]``, ``[B, C, 1, 1]`` or a single vector broadcast over B; ``feat``: the two maps of get_iou_feat
        (any ``[B, C, H, W]`` float32 map works; one that is not channels last is converted once).  The result is
        differentiable in ``proposals`` only: gradients to ``feat`` and ``modulation`` are None (the tracker never
        asks for them).  A box with a NaN, an infinity or a size <= 0 pools to zeros: its IoU is the head applied
        to zeros and its gradient zero.  ``B P == 0`` returns an empty tensor without a launch."""
        if isinstance(proposals, torch.Tensor) and not proposals.is_cuda:
            raise NotImplementedError("AtomIoUNet only supports GPU (cuda) tensors; there is no CPU path")
        if proposals.dtype != torch.float32:
            raise ValueError(f"proposals must be float32, got {proposals.dtype}")
        return _PredictIoU.apply(proposals, self, tuple(modulation), tuple(feat))

    def refine_boxes(self, modulation, feat, init_boxes, iters=5, step_length=1.0, step_decay=1.0):
        """``iters`` steps of the reference's box ascent (optimize_boxes_default), box += step * d iou / d box *
        (w, h, w, h) and step *= step_decay, in one library call -> (boxes ``[B, P, 4]``, iou ``[B, P]``), the IoU
        being the last forward's (of the boxes before the last update), as the reference returns it.
        ``step_length``: a number or a (position, size) pair."""
        self._cuda(init_boxes)
        B, P = init_boxes.shape[:2]
        out = init_boxes.detach().float().clone().contiguous()
        iou = torch.empty(B, P, dtype=torch.float32, device=out.device)
        if B * P == 0:
            return out, iou
        sp, ss = step_length if isinstance(step_length, (tuple, list)) else (step_length, step_length)
        head, fa, keep, need = self._args(modulation, feat, out)
        with torch.cuda.device(out.device):
            _rc(_lib.load().mmt_iounet_refine(ctypes.byref(head), ctypes.byref(fa), _p(keep[0]), _p(keep[1]), _p(out), P,
                                              int(iters), float(sp), float(ss), float(step_decay), _p(out), _p(iou),
                                              _p(self._ws(need)), need, _stream(out.device)), "mmt_iounet_refine")
        return out, iou
