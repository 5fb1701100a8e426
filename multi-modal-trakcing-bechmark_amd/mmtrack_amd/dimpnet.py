"""DeT / mfDiMP DiMP-50 classification path on the HIP kernels (mmt_conv2d_f32 & co, include/mmtrack.h).

``DiMPNet`` is DiMPnet_DeT with merge_type 'max' (RGBD/models/DeT/ltr/models/tracking/dimpnet.py:15-156,
built by dimp50_DeT, :421-476) as the DiMP tracker uses it (pytracking/tracker/dimp/dimp.py):

* ``extract_backbone(patches)``      NetWithBackbone.extract_backbone (net_wrappers.py:81-85): normalise
  each 3-channel half, two ResNet-50 backbones to layer3 (resnet.py), torch.max merge (dimpnet.py:103);
* ``extract_classification_feat``    the clf feature block (features.py:47-66: 3x3 conv 1024 -> 512 without
  bias, InstanceL2Norm) -> [N, 512, 18, 18] fp32 (NCHW, what the DiMP optimiser reads);
* ``init_filter(feat, bb)``          FilterInitializerLinear (initializer.py:118-170): 3x3 conv, PrRoIPool2D
  4 x 4 of the target box at 1/16, mean over the samples;
* ``classify``                       LinearFilter.classify (linear_filter.py:78-83) = dimp.apply_filter.

Weights load from the reference state_dict keys (load_state_dict strict on the keys this path reads;
IoU-Net ``bb_regressor.*``, ``layer4`` and ``fc`` keys are accepted and unused).  BatchNorm (eval) is
folded into each conv in float64 on the host.  Precision (``precision``): "f16x3" (default) runs every
convolution on the fp16 matrix cores with fp32-faithful split products (mmt_conv2d_f16x3, csrc/dimpconv.hip:
fp16 hi / lo halves of power-of-two range-scaled operands, Wh*Ah + Wl*Ah + Wh*Al with fp32 accumulation; the
activation scales come from each producing conv's max|y|, kept on the device); "fp32" keeps the plain fp32
MFMA kernel (mmt_conv2d_f32).  Everything else is fp32.  There is no CPU fallback: a missing libmmtrack.so
raises ImportError.
"""
from __future__ import annotations

import ctypes
import math
import os

from typing import NamedTuple

import torch

from . import _lib
from .dimp_table import IMAGE, OUT, layer_table, reference_rows, row_work
from .synth import RESNET50_LAYERS, dimp_shapes

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
_rc, _p, _stream = _lib.rc, _lib.ptr, _lib.stream


def range_scale(m):
    """engine_weights.cpp range_scale: the power of two s with m * s <= 2^14 (m > 0)."""
    return 2.0 ** (14 - math.ceil(math.log2(m))) if m > 0 else 1.0


MAX_WORDS = 64 * 32   # sharded max|y| words per tensor (mmt_conv_max_words)
# f16x3: the stem writes the max-pooled map directly (MMT_CONV_POOL); MMT_DIMP_STEMPOOL=0 (tuning A/B): the stem map
# and a separate max-pool launch
STEM_POOL = os.environ.get("MMT_DIMP_STEMPOOL", "1") != "0"


class _Conv:
    """One conv (+ folded BN): weight [Cout][kh][kw][Cin] and bias [Cout] fp32 on the device; with f16x3 the
    weights also as the fp16 halves of w * s_w, [Cout][Kp] (the stem: 4 channels per tap, K padded to 32)."""

    def __init__(self, w, bn=None, bias=None, stride=1, pad=0, dev=None, w4=True, f16x3=False):
        w = w.detach().double()
        co = w.shape[0]
        b = bias.detach().double() if bias is not None else torch.zeros(co, dtype=torch.float64)
        if bn is not None:
            g, beta, mean, var = (t.detach().double() for t in bn)
            s = g / torch.sqrt(var + 1e-5)
            w = w * s.view(-1, 1, 1, 1)
            b = (b - mean) * s + beta
        wk = w.permute(0, 2, 3, 1)
        # the 3-channel stem: weights padded to 4 channels per tap (MMT_CONV_W4, one float4 per tap)
        self.w4 = w4 and w.shape[1] == 3 and not os.environ.get("MMT_CONV_NOW4")   # (env: tuning A/B)
        if self.w4:
            wk = torch.nn.functional.pad(wk, (0, 1))
        self.w = wk.contiguous().float().to(dev)
        self.b = b.float().to(dev) if (bn is not None or bias is not None) else None
        self.cout, self.cin, self.kh, self.kw = co, w.shape[1], w.shape[2], w.shape[3]
        self.stride, self.pad = stride, pad
        self.f16x3 = f16x3
        if f16x3:
            wq = w.permute(0, 2, 3, 1)
            if self.cin == 3:
                wq = torch.nn.functional.pad(wq, (0, 1))
            wq = wq.reshape(co, -1).float()
            kp = (wq.shape[1] + 31) // 32 * 32
            wq = torch.nn.functional.pad(wq, (0, kp - wq.shape[1]))
            self.w_scale = range_scale(float(wq.abs().max()))
            v = wq * self.w_scale
            hi = v.half()
            lo = (v - hi.float()).half()
            self.wh, self.wl, self.kp = hi.contiguous().to(dev), lo.contiguous().to(dev), kp

    def out_hw(self, H, W):
        return (H + 2 * self.pad - self.kh) // self.stride + 1, (W + 2 * self.pad - self.kw) // self.stride + 1

    def group(self, x, out, relu=False, resid=None, merge_max=False, x_max=None, x_scale=0.0, y_max=None,
              pool=False):
        """This conv's operands as one mmt_conv_group of an f16x3 launch (pool: the stem with the 3 x 3 / stride-2
        max-pool fused, MMT_CONV_POOL; out is then the pooled map)."""
        flags = (1 if relu else 0) | (2 if merge_max else 0) | (8 if pool else 0)
        return _group(self, x.data_ptr(), out.data_ptr(), flags, _addr(resid), _addr(x_max), x_scale, _addr(y_max))

    def ws_need(self, lib, N, H, W, G, cin=None):
        """The split-K workspace bytes an f16x3 launch of G groups asks for (0: no split)."""
        return lib.mmt_conv2d_f16x3_ws_bytes(N, H, W, cin or self.cin, self.cout, self.kh, self.kw, self.stride,
                                             self.pad, G)

    def call(self, lib, groups, N, H, W, ws, need, cin=None):
        """One mmt_conv2d_f16x3_groups launch over groups, prepared for _launch; ws: the workspace pointer."""
        arr = (_lib.MmtConvGroup * len(groups))(*groups)
        return lib.mmt_conv2d_f16x3_groups, "mmt_conv2d_f16x3_groups", (
            arr, len(groups), N, H, W, cin or self.cin, self.kp, self.cout, self.kh, self.kw, self.stride, self.pad,
            ws, need)

    def call_f32(self, lib, x, N, H, W, out, relu=False, resid=None, merge_max=False):
        """The mmt_conv2d_f32 launch on the pointers x, out and resid, prepared for _launch."""
        flags = (1 if relu else 0) | (2 if merge_max else 0) | (4 if self.w4 else 0)
        return lib.mmt_conv2d_f32, "mmt_conv2d_f32", (
            x, N, H, W, self.cin, _p(self.w), _p(self.b), self.cout, self.kh, self.kw, self.stride, self.pad, resid,
            out, flags)

    def __call__(self, lib, x, N, H, W, out, stream, relu=False, resid=None, merge_max=False, x_max=None,
                 x_scale=0.0, y_max=None, ws=None):
        """f16x3: x_max = the input's sharded max words (or x_scale, a static power-of-two input scale), y_max =
        the output's (accumulated by the epilogue; None: not tracked); ws(nbytes) -> a device buffer for split-K
        partials (None: no split)."""
        if self.f16x3:
            run_f16x3(lib, self, [self.group(x, out, relu, resid, merge_max, x_max, x_scale, y_max)], N, H, W, ws,
                      stream)
        else:
            _launch(self.call_f32(lib, _p(x), N, H, W, _p(out), relu, _p(resid), merge_max), stream)
        return out


class _ConvDs:
    """A Bottleneck's conv3 (1 x 1) and its downsample (1 x 1 / stride) as one f16x3 GEMM over concatenated K
    (mmt_conv2d_f16x3_ds_groups, resnet.py:76-95): weights [Cout][Cin3 + Cin_d] -- conv3's BN-folded K then the
    downsample's -- split at one common scale, bias b3 + b_d; the downsample's output is never materialised."""

    def __init__(self, c3, ds, dev):
        w3 = c3.w.double().reshape(c3.cout, -1)     # [Cout][1][1][Cin] fp32 (BN folded) -> [Cout][Cin]
        wd = ds.w.double().reshape(ds.cout, -1)
        wq = torch.cat([w3, wd], dim=1).float()
        self.cout, self.cin3, self.cin_d, self.stride = c3.cout, c3.cin, ds.cin, ds.stride
        self.kp = wq.shape[1]
        self.w_scale = range_scale(float(wq.abs().max()))
        v = wq.to(dev) * self.w_scale
        hi = v.half()
        self.wh, self.wl = hi.contiguous(), (v - hi.float()).half().contiguous()
        self.b = (c3.b.double() + ds.b.double()).float().to(dev)

    def group(self, x, out, relu=True, x_max=None, y_max=None):
        return _group(self, x.data_ptr(), out.data_ptr(), 1 if relu else 0, None, _addr(x_max), 0.0, _addr(y_max))

    def ws_need(self, lib, N, H, W, G, cin=None):
        """As _Conv.ws_need (cin: not used, the weights fix K)."""
        return lib.mmt_conv2d_f16x3_ws_bytes(N, H, W, self.kp, self.cout, 1, 1, 1, 0, G)

    def call(self, lib, groups, ds, N, H, W, H2, W2, ws, need):
        """One mmt_conv2d_f16x3_ds_groups launch, prepared for _launch; ds: the addresses of (x2, its max words)
        per backbone; ws: the workspace pointer."""
        G = len(groups)
        arr = (_lib.MmtConvGroup * G)(*groups)
        darr = (_lib.MmtConvDs * G)(*[_lib.MmtConvDs(x2, x2m, 0.0) for x2, x2m in ds])
        return lib.mmt_conv2d_f16x3_ds_groups, "mmt_conv2d_f16x3_ds_groups", (
            arr, darr, G, N, H, W, self.cin3, H2, W2, self.cin_d, self.stride, self.kp, self.cout, ws, need)

    def run(self, lib, groups, ds, N, H, W, H2, W2, ws, stream):
        """groups: conv3's operands per backbone (x = conv2's output [N][H][W][Cin3]); ds: (x2 = the block input
        [N][H2][W2][Cin_d], its max words) per backbone."""
        need = self.ws_need(lib, N, H, W, len(groups))
        buf = ws(need) if (need and ws is not None) else None
        _launch(self.call(lib, groups, [(x2.data_ptr(), _addr(x2m)) for x2, x2m in ds], N, H, W, H2, W2, _p(buf),
                          need if buf is not None else 0), stream)


# f16x3: each stage's first Bottleneck runs conv3 + downsample as one GEMM (_ConvDs); MMT_DIMP_DSFUSE=0 (tuning A/B):
# the downsample conv writes its map and conv3 adds it as a residual
DS_FUSE = os.environ.get("MMT_DIMP_DSFUSE", "1") != "0"


def _addr(t):
    return t.data_ptr() if t is not None else None


def _group(conv, x, y, flags, resid=None, x_max=None, x_scale=0.0, y_max=None):
    """The weights of conv (a _Conv or a _ConvDs) and operands at device addresses as one mmt_conv_group."""
    return _lib.MmtConvGroup(x, conv.wh.data_ptr(), conv.wl.data_ptr(), conv.w_scale, _addr(conv.b), resid, y, x_max,
                             float(x_scale), y_max, flags)


def _launch(call, stream):
    """Run a prepared call (function, its name, its arguments but the stream) on stream."""
    fn, what, args = call
    _rc(fn(*args, stream), what)


def run_f16x3(lib, conv, groups, N, H, W, ws, stream, cin=None):
    """One mmt_conv2d_f16x3_groups launch of conv's shape over groups (the twin layers of the two backbones, or
    one); split-K partials in ws(nbytes) when the library asks for a split.  cin=4: the stem over an image
    padded to 4 channels (mmt_image_normalize4)."""
    need = conv.ws_need(lib, N, H, W, len(groups), cin)
    buf = ws(need) if (need and ws is not None) else None
    _launch(conv.call(lib, groups, N, H, W, _p(buf), need if buf is not None else 0, cin), stream)


class _Plan(NamedTuple):
    """The prepared launches of DiMPNet._backbones for one (N, H, W)."""
    calls: list            # (function, its name, its arguments but the stream), in launch order
    out_groups: list       # f16x3: the mmt_conv_group entries whose y is the returned layer3 map
    out_ptr: ctypes.c_void_p   # fp32: the pointer argument of the launches that write it
    out_max: object        # f16x3: the merged map's max words (slot 0)
    out_shape: tuple


class DiMPNet:
    def __init__(self, state_dict, device=None, out_dim=512, filter_size=4, feat_stride=16, precision="f16x3"):
        if precision not in ("f16x3", "fp32"):
            raise ValueError(f"precision must be 'f16x3' or 'fp32', got {precision!r}")
        self.precision = precision
        f16 = precision == "f16x3"
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("DiMPNet needs an MI355X (HIP device); there is no CPU path")
        self.dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        missing = [k for k in dimp_shapes() if not k.endswith("num_batches_tracked") and k not in state_dict]
        if missing:
            raise RuntimeError("Error(s) in loading state_dict: missing keys " + ", ".join(missing[:8]))
        for k, shp in dimp_shapes().items():
            if k in state_dict and tuple(state_dict[k].shape) != tuple(shp) and not k.endswith("predictor.weight") \
                    and not k.endswith("predictor.0.weight"):
                raise RuntimeError(f"Error(s) in loading state_dict: size mismatch for {k}: "
                                   f"{tuple(state_dict[k].shape)} vs {tuple(shp)}")
        sd = {k: torch.as_tensor(v) for k, v in state_dict.items()}
        self.sd_opt = {k[len("classifier.filter_optimizer."):]: v for k, v in sd.items()
                       if k.startswith("classifier.filter_optimizer.")}
        self.out_dim, self.filter_size, self.feat_stride = out_dim, filter_size, feat_stride
        self.norm_scale = math.sqrt(1.0 / (out_dim * filter_size * filter_size))

        def bn(pre):
            return [sd[pre + s] for s in (".weight", ".bias", ".running_mean", ".running_var")]
        self.convs = []   # per backbone: a dimp_table row's layer -> its _Conv ("<conv3>+ds": the fused _ConvDs)
        for fe in ("feature_extractor", "feature_extractor_depth"):
            cv = {"stem": _Conv(sd[fe + ".conv1.weight"], bn(fe + ".bn1"), stride=2, pad=3, dev=self.dev, f16x3=f16)}
            for li, (planes, nb, stride) in enumerate(RESNET50_LAYERS):
                for b in range(nb):
                    name = f"layer{li + 1}.{b}"
                    pre, s = f"{fe}.{name}", stride if b == 0 else 1
                    cv[name + ".conv1"] = _Conv(sd[pre + ".conv1.weight"], bn(pre + ".bn1"), dev=self.dev, f16x3=f16)
                    cv[name + ".conv2"] = _Conv(sd[pre + ".conv2.weight"], bn(pre + ".bn2"), stride=s, pad=1,
                                                dev=self.dev, f16x3=f16)
                    c3 = cv[name + ".conv3"] = _Conv(sd[pre + ".conv3.weight"], bn(pre + ".bn3"), dev=self.dev,
                                                     f16x3=f16)
                    if b == 0:
                        ds = cv[name + ".downsample"] = _Conv(sd[pre + ".downsample.0.weight"],
                                                              bn(pre + ".downsample.1"), stride=s, dev=self.dev,
                                                              f16x3=f16)
                        if f16:
                            cv[name + ".conv3+ds"] = _ConvDs(c3, ds, self.dev)
            self.convs.append(cv)
        self.clf = _Conv(sd["classifier.feature_extractor.0.weight"], pad=1, dev=self.dev, f16x3=f16)
        self.fconv = _Conv(sd["classifier.filter_initializer.filter_conv.weight"], pad=1,
                           bias=sd["classifier.filter_initializer.filter_conv.bias"], dev=self.dev, f16x3=f16)
        # f16x3 activation range: sharded max|y| words per produced tensor, zeroed once per extract_backbone;
        # the normalised image and the InstanceL2Norm output have static bounds
        self._max_words = torch.zeros(128 * MAX_WORDS, dtype=torch.float32, device=self.dev) if f16 else None
        self.image_scale = range_scale(max((1 - m) / s for m, s in zip(MEAN, STD)))
        self.l2_scale = lambda L: range_scale(self.norm_scale * math.sqrt(L))
        self._mean = (ctypes.c_float * 3)(*MEAN)
        self._std = (ctypes.c_float * 3)(*STD)
        self._bufs = {}
        self._plans = {}   # (N, H, W, STEM_POOL, DS_FUSE) -> _Plan; emptied when a buffer is replaced

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return _stream(self.dev)

    def _buf(self, name, n):
        b = self._bufs.get(name)
        if b is None or b.numel() < n:
            if b is not None:   # the plans hold the old buffer's address
                self._plans.clear()
            b = self._bufs[name] = torch.empty(n, dtype=torch.float32, device=self.dev)
        return b[:n]

    def _ws(self, nbytes):
        return self._buf("splitk", (nbytes + 3) // 4)

    def _plan(self, N, H, W):
        """The prepared launches of both ResNet-50s to layer3 on N images of H x W (dimp_table.layer_table with
        this module's STEM_POOL / DS_FUSE): buffers at their final size, group arrays filled in, each launch's
        split-K workspace asked of the library once.  The rows writing the merged layer3 map get its address per
        forward pass (_backbones)."""
        key = (N, H, W, STEM_POOL, DS_FUSE)
        if key in self._plans:
            return self._plans[key]
        lib, f16, K = self.lib, self.precision == "f16x3", range(len(self.convs))
        tab = layer_table(H, W, self.precision, STEM_POOL, DS_FUSE, len(K))
        if f16 and tab.nslots * MAX_WORDS > self._max_words.numel():
            raise RuntimeError("DiMPNet: out of max-word slots")
        convs = [[self.convs[k].get(r.layer + ("+ds" if r.kind == "conv_ds" else "")) for k in r.backbones]
                 for r in tab.rows]   # per row and backbone (a max-pool: None)
        for r, cs in zip(tab.rows, convs):   # a launch takes its shape from the conv, its buffers' sizes from the row
            for c in (cs if r.kind != "pool" else ()):
                if r.kind == "conv_ds":
                    same = (c.cout, c.cin3, c.cin_d, c.stride) == (r.cout, r.cin, r.x2_cin, r.x2_stride)
                else:   # the f16x3 stem reads the image padded to 4 channels
                    same = (c.cout, c.cin + (f16 and r.layer == "stem"), c.kh, c.kw, c.stride, c.pad) == \
                        (r.cout, r.cin, r.k, r.k, r.stride, r.pad)
                if not same:
                    raise RuntimeError(f"DiMPNet: the weights of {r.layer} do not have the layer table's shape")
        needs = [cs[0].ws_need(lib, N, r.H, r.W, len(cs), r.cin) if f16 and r.kind != "pool" else 0
                 for r, cs in zip(tab.rows, convs)]
        ws = _p(self._ws(max(needs))) if max(needs) else None
        addr = {(name, k): self._buf(("xa", "xb")[k] if name == IMAGE else f"{name}{k}", N * n).data_ptr()
                for name, n in tab.buffers.items() for k in K}
        words = (lambda slot: self._max_words.data_ptr() + 4 * MAX_WORDS * slot if isinstance(slot, int) else None)
        last = tab.rows[-1]
        plan = _Plan([], [], ctypes.c_void_p(), self._max_words[:MAX_WORDS] if f16 else None,
                     (N, last.Ho, last.Wo, last.cout))
        for r, cs, need in zip(tab.rows, convs, needs):
            at = (lambda name, i: addr.get((name, r.backbones[i])))   # None: no such operand, or OUT (set per pass)
            if r.kind == "pool" or not f16:
                x, resid = ctypes.c_void_p(at(r.x, 0)), ctypes.c_void_p(at(r.resid, 0))
                y = plan.out_ptr if r.y == OUT else ctypes.c_void_p(at(r.y, 0))
                call = (lib.mmt_maxpool2d_f32, "mmt_maxpool2d_f32", (x, N, r.H, r.W, r.cin, r.k, r.stride, r.pad, y)) \
                    if r.kind == "pool" else cs[0].call_f32(lib, x, N, r.H, r.W, y, r.relu, resid, r.merge_max)
            else:
                flags = (1 if r.relu else 0) | (2 if r.merge_max else 0) | (8 if r.pool else 0)
                groups = [_group(c, at(r.x, i), at(r.y, i), flags, at(r.resid, i), words(r.x_slot[i]),
                                 self.image_scale if r.x_slot[i] == IMAGE else 0.0, words(r.y_slot[i]))
                          for i, c in enumerate(cs)]
                if r.kind == "conv_ds":
                    call = cs[0].call(lib, groups, [(at(r.x2, i), words(r.x2_slot[i])) for i in range(len(cs))], N, r.H,
                                      r.W, r.x2_H, r.x2_W, ws if need else None, need)
                else:
                    call = cs[0].call(lib, groups, N, r.H, r.W, ws if need else None, need, r.cin)
                if r.y == OUT:
                    plan.out_groups.append(call[2][0][0])   # the group array's entry: a view, not a copy
            plan.calls.append(call)
        self._plans[key] = plan
        return plan

    def flops(self, H=288, W=288):
        """Algorithmic FLOPs (2 x MACs) of extract_backbone + extract_classification_feat for one [6, H, W] image."""
        return sum(f for f, _ in self.layer_work(H, W))

    def layer_work(self, H=288, W=288):
        """(FLOPs, minimum HBM bytes) of every conv and max-pool of extract_backbone + the clf conv for one
        [6, H, W] image (dimp_table.row_work: each layer's input read once, its output written once and read back
        by the MAX merge, the residual read, fp32 activations; f16x3 weights (hi + lo) are read once per launch --
        amortised over the batch, so not counted per image).  The per-layer roofline of a batch is the sum over
        layers of max(FLOPs / matrix peak, bytes / HBM bandwidth).  (The reference's layers as the yardstick: the
        fused conv3 + downsample of the f16x3 path moves fewer bytes than the two layers it replaces.)"""
        return [row_work(r) for r in reference_rows(H, W, len(self.convs), self.clf.cout)]

    def roofline_ms(self, n, peak_tflops, hbm_tbps, H=288, W=288):
        """The per-layer roofline time (ms) of extract_backbone + clf conv over a batch of n images."""
        return sum(max(n * f / (peak_tflops * 1e12), n * b / (hbm_tbps * 1e12)) for f, b in self.layer_work(H, W)) * 1e3

    # ------------------------------------------------------------------ the network's tracker-side entry points
    def extract_backbone(self, im):
        """im: [N, 6, H, W] fp32 CUDA pixel values (0..255) -> merged layer3 NHWC [N, H/16, W/16, 1024]."""
        if not (isinstance(im, torch.Tensor) and im.is_cuda and im.dtype == torch.float32 and im.dim() == 4
                and im.shape[1] == 6):
            raise ValueError("im must be an [N, 6, H, W] float32 CUDA tensor")
        im = im.contiguous()
        N, _, H, W = im.shape
        s = self._stream()
        f16 = self.precision == "f16x3"
        pc = 4 if f16 else 3   # f16x3: pixels padded to 4 channels (one 16-B load per stem tap)
        xa = self._buf("xa", N * H * W * pc)
        xb = self._buf("xb", N * H * W * pc)
        norm = self.lib.mmt_image_normalize4 if f16 else self.lib.mmt_image_normalize
        _rc(norm(_p(im), N, 6, H, W, self._mean, self._std, _p(xa), _p(xb), s), "mmt_image_normalize")
        return self._backbones(N, H, W, s)

    def norm4_buffers(self, N, H, W):
        """f16x3: the two normalised 4-channel NHWC halves [N*H*W*4] that extract_backbone_norm4 reads (a sampler
        that normalises, mmt_dimp_track_sample_norm4, writes them directly)."""
        if self.precision != "f16x3":
            raise ValueError("norm4 buffers: f16x3 only")
        return self._buf("xa", N * H * W * 4), self._buf("xb", N * H * W * 4)

    def max_words(self):
        """f16x3: the device words of every tensor's sharded max|y| (zeroed before each extract_backbone)."""
        return self._max_words

    def extract_backbone_norm4(self, N, H, W, words_cleared=False):
        """extract_backbone on the patches already normalised into norm4_buffers(N, H, W); words_cleared: the
        max words were zeroed by an earlier launch on the stream (the normalising sampler)."""
        self.norm4_buffers(N, H, W)
        return self._backbones(N, H, W, self._stream(), words_cleared)

    def _backbones(self, N, H, W, s, words_cleared=False):
        """Both ResNet-50s to layer3 on the normalised halves in the "xa" / "xb" buffers: the RGB backbone's last
        conv writes the returned map [N, H/16, W/16, 1024], the aux backbone's max-merges into it (dimpnet.py:103).
        f16x3: every conv reads its input's max words and accumulates its output's; slot 0, shared by the two last
        convs, bounds the merged map."""
        plan = self._plan(N, H, W)
        out = torch.empty(plan.out_shape, dtype=torch.float32, device=self.dev)
        if self._max_words is not None and not words_cleared:
            self._max_words.zero_()
        plan.out_ptr.value = out.data_ptr()   # fp32 launches
        for g in plan.out_groups:             # f16x3 launches
            g.y = out.data_ptr()
        for call in plan.calls:
            _launch(call, s)
        self._layer3_max = (out, plan.out_max)
        return out

    def extract_classification_feat(self, layer3, nhwc=False):
        """layer3 NHWC [N, h, w, 1024] -> clf features [N, 512, h, w] (and the NHWC copy when nhwc=True)."""
        N, h, w, _ = layer3.shape
        s = self._stream()
        t = self._buf("clf", N * h * w * self.out_dim)
        lm = getattr(self, "_layer3_max", None)
        if self.precision == "f16x3" and (lm is None or lm[0] is not layer3):
            raise ValueError("f16x3: extract_classification_feat takes the layer3 map of the last extract_backbone")
        self.clf(self.lib, layer3, N, h, w, t, s, x_max=lm[1] if lm else None, ws=self._ws)
        out = torch.empty(N, self.out_dim, h, w, dtype=torch.float32, device=self.dev)
        out_nhwc = torch.empty(N, h, w, self.out_dim, dtype=torch.float32, device=self.dev) if nhwc else None
        l2ws = self._buf("l2ws", (self.lib.mmt_instance_l2norm_ws_bytes(N, h, w) + 3) // 4)
        _rc(self.lib.mmt_instance_l2norm(_p(t), N, h, w, self.out_dim, self.norm_scale, 1e-5, _p(out_nhwc), _p(out),
                                         _p(l2ws), s), "mmt_instance_l2norm")
        return (out, out_nhwc) if nhwc else out

    def init_filter(self, feat_nhwc, bb):
        """feat_nhwc [N, h, w, 512] (extract_classification_feat(..., nhwc=True)[1]); bb [N, 4] xywh (sample
        coordinates) -> filter [1, 512, fs, fs]."""
        N, h, w, C = feat_nhwc.shape
        s = self._stream()
        f = self._buf("fconv", N * h * w * C)
        # the InstanceL2Norm output: |y| <= norm_scale * sqrt(C h w) (normalization.py:6-21)
        self.fconv(self.lib, feat_nhwc, N, h, w, f, s, x_scale=self.l2_scale(C * h * w), ws=self._ws)
        bb = torch.as_tensor(bb, dtype=torch.float32).reshape(-1, 4).clone()
        bb[:, 2:4] = bb[:, 0:2] + bb[:, 2:4]
        rois = bb.to(self.dev)
        fs = self.filter_size
        pooled = torch.empty(N, C, fs, fs, dtype=torch.float32, device=self.dev)
        _rc(self.lib.mmt_prroi_pool(_p(f), N, h, w, C, _p(rois), 1.0 / self.feat_stride, fs, fs, _p(pooled), s),
            "mmt_prroi_pool")
        return pooled.mean(0, keepdim=True) if N > 1 else pooled

    def classify(self, weights, feat):
        from .dimp import apply_filter
        return apply_filter(feat.reshape(-1, 1, *feat.shape[-3:]), weights)


def sample_patch_device(frame, geom, out_hw):
    """mmt_sample_patch: frame H x W x C uint8 CUDA tensor, geom (df, os_y, os_x, tl_y, tl_x, sz_h, sz_w)
    -> [1, C, out_h, out_w] fp32 CUDA tensor."""
    lib = _lib.load()
    H, W, C = frame.shape
    out = torch.empty(1, C, int(out_hw[0]), int(out_hw[1]), dtype=torch.float32, device=frame.device)
    g = (ctypes.c_int * 7)(*[int(v) for v in geom])
    _rc(lib.mmt_sample_patch(_p(frame), H, W, C, frame.stride(0), g, int(out_hw[0]), int(out_hw[1]), _p(out),
                             _stream(frame.device)), "mmt_sample_patch")
    return out


def patch_transform_device(img, tf, out_hw):
    """mmt_patch_transform of a [1, C, E_h, E_w] fp32 CUDA patch with one _lib.MmtPatchTf -> [1, C, oh, ow]."""
    lib = _lib.load()
    _, C, Eh, Ew = img.shape
    img = img.contiguous()
    out = torch.empty(1, C, int(out_hw[0]), int(out_hw[1]), dtype=torch.float32, device=img.device)
    _rc(lib.mmt_patch_transform(_p(img), C, Eh, Ew, ctypes.byref(tf), int(out_hw[0]), int(out_hw[1]), _p(out),
                                _stream(img.device)),
        "mmt_patch_transform")
    return out


def conv2d(x_nchw, w, bias=None, stride=1, pad=0, resid=None, relu=False, w4=True, precision="fp32", x_max=None,
           y_max=None, split=False, merge_into=None):
    """Test / tool helper: torch NCHW conv through mmt_conv2d_f32 or (precision "f16x3") mmt_conv2d_f16x3
    (weights nn.Conv2d layout; f16x3 input range: x_max words, else the static scale of max|x|; split: give the
    library a split-K workspace; merge_into: an NHWC map the output is max-merged into (and returned))."""
    lib = _lib.load()
    f16 = precision == "f16x3"
    conv = _Conv(w, bias=bias, stride=stride, pad=pad, dev=x_nchw.device, w4=w4, f16x3=f16)
    N, C, H, W = x_nchw.shape
    Ho, Wo = conv.out_hw(H, W)
    x = x_nchw.permute(0, 2, 3, 1).contiguous()
    out = merge_into if merge_into is not None else torch.empty(N, Ho, Wo, conv.cout, dtype=torch.float32,
                                                                device=x.device)
    r = resid.permute(0, 2, 3, 1).contiguous() if resid is not None else None
    kw = {}
    if f16:
        kw = dict(x_max=x_max, x_scale=0.0 if x_max is not None else range_scale(float(x.abs().max())), y_max=y_max)
        if split:
            kw["ws"] = lambda n: torch.empty((n + 3) // 4, dtype=torch.float32, device=x.device)
    conv(lib, x, N, H, W, out, _stream(x.device), relu=relu, resid=r,
         merge_max=merge_into is not None, **kw)
    return out.permute(0, 3, 1, 2)


def prroi_pool(feat_nchw, rois_xyxy, spatial_scale, ph, pw):
    """Test helper: PrRoIPool2D of roi n on image n."""
    lib = _lib.load()
    N, C, H, W = feat_nchw.shape
    f = feat_nchw.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(N, C, ph, pw, dtype=torch.float32, device=f.device)
    r = torch.as_tensor(rois_xyxy, dtype=torch.float32).reshape(N, 4).to(f.device)
    _rc(lib.mmt_prroi_pool(_p(f), N, H, W, C, _p(r), spatial_scale, ph, pw, _p(out),
                           _stream(f.device)), "mmt_prroi_pool")
    return out


__all__ = ["DiMPNet", "sample_patch_device", "patch_transform_device", "conv2d", "prroi_pool"]
