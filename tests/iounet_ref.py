"""AtomIoUNet restated in differentiable torch (a test helper, not an oracle module), on top of tests/prroi_ref.py.

Written from the math of ltr/models/bbreg/atom_iou_net.py: conv + BatchNorm (eval, eps 1e-5) + ReLU blocks, Precise
RoI Pooling of the modulated maps (5 x 5 at 1/8 and 3 x 3 at 1/16 for the proposals, 3 x 3 and 1 x 1 for the target
box), two linear + BatchNorm + ReLU blocks and a linear IoU predictor; and the box ascent of
pytracking/tracker/dimp/dimp.py:727-752, box += step * d iou / d box * (w, h, w, h).  Everything runs in the dtype
asked for, so the same code is the float64 reference of the GPU tests and, in float32 on the CPU, the measure of
float32's own error that sets their bars.  It also reports the hidden layers' pre-activations, for the ReLU-kink
condition of tests/test_iounet_ref.py.

``inputs(...)`` makes the seeded inputs every IoU-Net test regenerates instead of storing.
"""
import torch
import torch.nn.functional as F

from tests.prroi_ref import prroi_pool_ref

EPS = 1e-5


class IoUNetRef:
    def __init__(self, state_dict, prefix="bb_regressor.", dtype=torch.float64):
        self.dt = dtype
        self.sd = {k[len(prefix):]: v.to(dtype) if v.is_floating_point() else v
                   for k, v in state_dict.items() if k.startswith(prefix)}
        self.pre = []          # (smallest |pre-activation| / largest, per hidden layer) of every predict_iou call

    def _bn(self, x, pre):
        s = self.sd
        shape = (1, -1) + (1,) * (x.dim() - 2)
        inv = s[pre + ".weight"] / torch.sqrt(s[pre + ".running_var"] + EPS)
        return (x - s[pre + ".running_mean"].view(shape)) * inv.view(shape) + s[pre + ".bias"].view(shape)

    def _conv(self, x, name, pad):
        y = F.conv2d(x, self.sd[name + ".0.weight"], self.sd[name + ".0.bias"], padding=pad)
        return F.relu(self._bn(y, name + ".1"))

    def _linear(self, x, name):
        y = F.linear(x.reshape(x.shape[0], -1), self.sd[name + ".linear.weight"], self.sd[name + ".linear.bias"])
        return self._bn(y, name + ".bn")   # the pre-activation: the block's output is its ReLU

    @staticmethod
    def _rois(boxes):
        """boxes [B, P, 4] xywh -> [B P, 5] (sequence, x0, y0, x1, y1)."""
        B, P = boxes.shape[:2]
        idx = torch.arange(B, dtype=boxes.dtype).view(B, 1, 1).expand(B, P, 1)
        return torch.cat([idx, boxes[..., :2], boxes[..., :2] + boxes[..., 2:]], dim=2).reshape(-1, 5)

    def get_iou_feat(self, feats):
        f3, f4 = (f.to(self.dt) for f in feats)
        return (self._conv(self._conv(f3, "conv3_1t", 1), "conv3_2t", 1),
                self._conv(self._conv(f4, "conv4_1t", 1), "conv4_2t", 1))

    def get_modulation(self, feats, bb):
        f3, f4 = (f.to(self.dt) for f in feats)
        rois = self._rois(bb.to(self.dt).reshape(-1, 1, 4))
        r3 = prroi_pool_ref(self._conv(f3, "conv3_1r", 1), rois, 3, 3, 1 / 8)
        r4 = prroi_pool_ref(self._conv(f4, "conv4_1r", 1), rois, 1, 1, 1 / 16)
        both = torch.cat([self._conv(r3, "fc3_1r", 0), r4], dim=1)
        return self._conv(both, "fc34_3r", 0), self._conv(both, "fc34_4r", 0)

    def predict_iou(self, modulation, feat, proposals):
        """modulation: two [B, C] (or [B, C, 1, 1]); feat: two [B, C, H, W]; proposals [B, P, 4] -> [B, P]."""
        B, P = proposals.shape[:2]
        rois = self._rois(proposals.to(self.dt))
        hidden = []
        for m, f, name, bins, scale in zip(modulation, feat, ("fc3_rt", "fc4_rt"), (5, 3), (1 / 8, 1 / 16)):
            att = f.to(self.dt) * m.to(self.dt).reshape(B, -1, 1, 1)
            hidden.append(self._linear(prroi_pool_ref(att, rois, bins, bins, scale), name))
        self.pre.append(tuple(float(h.detach().abs().min() / h.detach().abs().max()) for h in hidden))
        h = F.relu(torch.cat(hidden, dim=1))
        return F.linear(h, self.sd["iou_predictor.weight"], self.sd["iou_predictor.bias"]).reshape(B, P)

    def iou_and_grad(self, modulation, feat, proposals, gradient=None):
        """(iou [B, P], d sum(gradient * iou) / d proposals [B, P, 4]); gradient None: ones."""
        bb = proposals.to(self.dt).clone().requires_grad_(True)
        iou = self.predict_iou(modulation, feat, bb)
        g = torch.ones_like(iou) if gradient is None else gradient.to(self.dt)
        grad, = torch.autograd.grad((iou * g).sum(), bb)
        return iou.detach(), torch.nan_to_num(grad, nan=0.0)

    def refine(self, modulation, feat, boxes, iters=5, step_length=1.0, step_decay=1.0):
        """The ascent: (boxes after each step [iters, B, P, 4], the last forward's iou [B, P])."""
        step = torch.tensor([step_length[0], step_length[0], step_length[1], step_length[1]], dtype=self.dt) \
            if isinstance(step_length, (tuple, list)) else torch.full((4,), float(step_length), dtype=self.dt)
        out, trace, iou = boxes.to(self.dt), [], None
        for _ in range(iters):
            iou, grad = self.iou_and_grad(modulation, feat, out)
            out = out + step * grad * out[..., 2:].repeat(1, 1, 2)
            trace.append(out)
            step = step * step_decay
        return torch.stack(trace), iou


def inputs(seed, B, P, size, input_dim=None, pooled=(256, 256)):
    """Seeded float32 inputs on an image of size x size pixels (maps size / 8 and size / 16): the IoU feature maps
    ``feat`` ([B, pooled[i], h, w], post-ReLU like), positive modulation vectors ``mod`` ([B, pooled[i]]), a target
    box ``bb`` [B, 4] and ``boxes`` [B, P, 4] scattered around it (xywh, image coordinates); with ``input_dim`` also
    the backbone maps ``back`` ([B, input_dim[i], h, w]) the convs read."""
    g = torch.Generator().manual_seed(1000 + seed)
    h3, h4 = size // 8, size // 16
    out = {}
    out["feat"] = [torch.randn(B, pooled[0], h3, h3, generator=g).relu(), torch.randn(B, pooled[1], h4, h4, generator=g).relu()]
    out["mod"] = [torch.rand(B, pooled[0], generator=g) + 0.25, torch.rand(B, pooled[1], generator=g) + 0.25]
    centre = size * (0.5 + 0.1 * (torch.rand(B, 2, generator=g) - 0.5))
    wh = size * (0.22 + 0.12 * torch.rand(B, 2, generator=g))
    out["bb"] = torch.cat([centre - wh / 2, wh], dim=1)
    jitter = (torch.rand(B, P, 4, generator=g) - 0.5) * size * torch.tensor([0.08, 0.08, 0.1, 0.1])
    out["boxes"] = out["bb"][:, None, :] + jitter
    if input_dim is not None:
        out["back"] = [torch.randn(B, input_dim[0], h3, h3, generator=g).relu(),
                       torch.randn(B, input_dim[1], h4, h4, generator=g).relu()]
    return out


# ----------------------------------------------------------------------------- the cases of the IoU-Net tests
HEADS = {"real": dict(pooled=(256, 256), inter=(256, 256)),     # Kd 6400 / 2304
         "small": dict(pooled=(72, 40), inter=(48, 80))}         # Kd 1800 / 360: a K tail and a partial N tile
GOLDEN = dict(seed=4, B=2, P=10, size=288, input_dim=(512, 1024), iters=5)


def head_state_dict(head, seed):
    """Seeded weights with the named head (the convs at a small input_dim: the head's weights depend on the seed and
    their own shapes only)."""
    from mmtrack_amd import synth
    h = HEADS[head]
    return synth.make_iounet_state_dict(seed, input_dim=(32, 32), pred_input_dim=h["pooled"], pred_inter_dim=h["inter"])


# Every input on which a GPU result is compared with this restatement in float64: (head, B, P) -> seed of the weights
# and the inputs, on a 96-pixel image (maps 12 x 12 and 6 x 6).  The seeds are chosen so that the ReLU-kink condition
# of tests/test_iounet_ref.py holds (mostly the first from 1 upwards that does).
PREDICT_CASES = {
    ("real", 1, 1): 1, ("real", 1, 10): 1, ("real", 1, 17): 4, ("real", 3, 1): 1, ("real", 3, 10): 4, ("real", 3, 17): 3,
    ("small", 1, 1): 1, ("small", 1, 10): 1, ("small", 1, 17): 1, ("small", 3, 1): 1, ("small", 3, 10): 1,
    ("small", 3, 17): 2,
}
# the ascents compared with float64: (head, step_length, step_decay) -> seed; B = 2, P = 10, 5 steps, 96 pixels.  The
# maps are 12 x 12 noise, far steeper than the golden's conv outputs, so the step is 0.2 (boxes move 5 to 15 pixels).
REFINE_CASES = {("real", 0.2, 1.0): 24, ("real", (0.2, 0.1), 0.5): 7, ("small", 0.2, 1.0): 1, ("small", (0.2, 0.1), 0.5): 1}
REFINE_B, REFINE_P, REFINE_ITERS, SMALL_SIZE = 2, 10, 5, 96
