"""Precise RoI Pooling with both gradients, on the HIP kernels of csrc/prroi.hip.

``prroi_pool2d`` and ``PrRoIPool2D`` keep the contract of the reference's
``ltr/external/PreciseRoIPooling/pytorch/prroi_pool`` (functional.py, prroi_pool.py), whose CUDA extension cannot be
built on an MI355X: float32 GPU tensors in, ``[K, C, PH, PW]`` out, gradients to the features and to the box
coordinates (what IoU-Net's box refinement ascends on).  There is no CPU path: a CPU tensor raises
NotImplementedError as the reference does, and a missing library is an ImportError.
"""
import torch
from torch import nn

from . import _lib

__all__ = ["prroi_pool2d", "PrRoIPool2D"]


def _channels_last(features):
    """features [N, C, H, W] -> (tensor to read, (pixel, row, image) pitches in floats).  A tensor whose channel
    stride is 1 and whose other strides the kernels can walk (a channels_last tensor, or a channel / column slice of
    a wider one) is read in place; any other layout is converted once."""
    n, c, h, w = features.shape
    sn, sc, sh, sw = features.stride()
    row_extent = (w - 1) * sw + c
    if (sc == 1 and sw >= c and sh >= row_extent and sn >= (h - 1) * sh + row_extent
            and sw % 4 == 0 and sh % 4 == 0 and sn % 4 == 0 and features.data_ptr() % 16 == 0):
        return features, (sw, sh, sn)
    f = features.contiguous(memory_format=torch.channels_last)
    return f, (c, w * c, h * w * c)


class PrRoIPool2DFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, pooled_height, pooled_width, spatial_scale):
        assert "FloatTensor" in features.type() and "FloatTensor" in rois.type(), \
            "Precise RoI Pooling only takes float input, got {} for features and {} for rois.".format(
                features.type(), rois.type())
        if not (features.is_cuda and rois.is_cuda):
            raise NotImplementedError("Precise RoI Pooling only supports GPU (cuda) implememtations.")
        if features.dim() != 4 or rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError(f"features must be [N, C, H, W] and rois [K, 5], got {tuple(features.shape)} and "
                             f"{tuple(rois.shape)}")
        if rois.device != features.device:
            raise ValueError("features and rois are on different devices")
        ph, pw, scale = int(pooled_height), int(pooled_width), float(spatial_scale)
        n, c, h, w = features.shape
        k = rois.shape[0]
        ctx.params = (ph, pw, scale)
        ctx.nchw = features.is_contiguous() and not features.is_contiguous(memory_format=torch.channels_last)
        out = torch.empty((k, c, ph, pw), dtype=torch.float32, device=features.device)
        if k == 0:
            ctx.save_for_backward(features, rois, out)
            ctx.pitches = None
            return out
        f, pitches = _channels_last(features.detach())
        r = rois.detach().contiguous()
        lib = _lib.load()
        with torch.cuda.device(features.device):
            _lib.rc(lib.mmt_prroi_pool_rois(_lib.ptr(f), n, h, w, c, *pitches, _lib.ptr(r), k, scale, ph, pw,
                                            _lib.ptr(out), _lib.stream(features.device)), "mmt_prroi_pool_rois")
        ctx.pitches = pitches
        ctx.save_for_backward(f, r, out)
        return out

    @staticmethod
    def backward(ctx, grad_output):
        f, r, out = ctx.saved_tensors
        ph, pw, scale = ctx.params
        n, c, h, w = f.shape
        k = r.shape[0]
        grad_features = grad_rois = None
        if k == 0:
            if ctx.needs_input_grad[0]:
                grad_features = torch.zeros_like(f)
            if ctx.needs_input_grad[1]:
                grad_rois = torch.zeros_like(r)
            return grad_features, grad_rois, None, None, None
        lib = _lib.load()
        g = grad_output.contiguous()
        with torch.cuda.device(f.device):
            s = _lib.stream(f.device)
            if ctx.needs_input_grad[0]:
                gf = torch.empty((n, h, w, c), dtype=torch.float32, device=f.device)
                _lib.rc(lib.mmt_prroi_pool_rois_grad_feat(n, h, w, c, _lib.ptr(r), k, scale, ph, pw, _lib.ptr(g),
                                                          _lib.ptr(gf), s), "mmt_prroi_pool_rois_grad_feat")
                grad_features = gf.permute(0, 3, 1, 2)   # the channels_last view of the NHWC buffer
                if ctx.nchw:
                    grad_features = grad_features.contiguous()
            if ctx.needs_input_grad[1]:
                grad_rois = torch.empty((k, 5), dtype=torch.float32, device=f.device)
                _lib.rc(lib.mmt_prroi_pool_rois_grad_rois(_lib.ptr(f), n, h, w, c, *ctx.pitches, _lib.ptr(r), k, scale,
                                                          ph, pw, _lib.ptr(out), _lib.ptr(g), _lib.ptr(grad_rois), s),
                        "mmt_prroi_pool_rois_grad_rois")
        return grad_features, grad_rois, None, None, None


def prroi_pool2d(features, rois, pooled_height, pooled_width, spatial_scale):
    """Precise RoI Pooling: ``features`` float32 ``[N, C, H, W]`` and ``rois`` float32 ``[K, 5]`` (batch index, x0,
    y0, x1, y1 in image coordinates), both on the GPU, to ``[K, C, pooled_height, pooled_width]``.

    Differentiable in ``features`` and in ``rois`` (column 0 of the box gradient is 0); each gradient is computed only
    if required.  ``features`` in ``torch.channels_last`` (or any view with channel stride 1 and 16-byte aligned
    pixel, row and image strides) are read in place; any other layout is converted once with
    ``.contiguous(memory_format=torch.channels_last)``, and ``grad_features`` comes back in the input's memory format.
    ``C`` must be a multiple of 4 and the pooled sizes 1..8 (ValueError otherwise).  The launches are ordered on
    torch's current stream.  ``K == 0`` returns an empty tensor without a launch.  A ROI with a non-finite value, an
    index outside ``[0, N)`` or no area pools to zeros with zero gradients; no ROI value makes a kernel read outside
    the map.  A dtype other than float32 fails the reference's assertion; a CPU tensor raises NotImplementedError.
    """
    return PrRoIPool2DFunction.apply(features, rois, pooled_height, pooled_width, spatial_scale)


class PrRoIPool2D(nn.Module):
    """``prroi_pool2d`` with fixed pooled size and spatial scale (the reference's module of the same name)."""

    def __init__(self, pooled_height, pooled_width, spatial_scale):
        super().__init__()
        self.pooled_height = int(pooled_height)
        self.pooled_width = int(pooled_width)
        self.spatial_scale = float(spatial_scale)

    def forward(self, features, rois):
        return prroi_pool2d(features, rois, self.pooled_height, self.pooled_width, self.spatial_scale)

    def extra_repr(self):
        return f"kernel_size=({self.pooled_height}, {self.pooled_width}), spatial_scale={self.spatial_scale}"
