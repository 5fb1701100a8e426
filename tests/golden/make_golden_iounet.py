"""Generate tests/golden/iounet_det.npz by running the REFERENCE AtomIoUNet (RGBD/models/DeT:
ltr/models/bbreg/atom_iou_net.py, input_dim (512, 1024) as dimp50_DeT builds it) in float64 on the CPU, on seeded
synthetic weights (mmtrack_amd.synth.make_iounet_state_dict) and the seeded inputs of tests/iounet_ref.inputs, and
the REFERENCE box ascent, pytracking/tracker/dimp/dimp.py DiMP.optimize_boxes_default, called on a stub ``self``
(params, net.bb_regressor, iou_modulation), so its update rule is what the file pins.

Build container only (needs the reference tree); the stand-ins are make_golden_dimp.install()'s, and the reference's
three PrRoIPool2D modules (a CUDA extension) are replaced by tests/prroi_ref.prroi_pool_ref, the restatement the
operator's own tests pin.  Stored: the modulation vectors, every 16th channel of the two IoU feature maps, IoU and box
gradient at the initial boxes, the boxes after each of the 5 steps (optimize_boxes_default run with 1..5 iterations),
the IoU it returns, and the smallest |pre-activation| of the two hidden layers relative to the layer's largest, over
all steps.

Usage:  python tests/golden/make_golden_iounet.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import make_golden_dimp as mgd  # noqa: E402
from mmtrack_amd import synth  # noqa: E402
from tests.iounet_ref import GOLDEN, inputs  # noqa: E402
from tests.prroi_ref import prroi_pool_ref  # noqa: E402

SEED, B, P, SIZE, ITERS = (GOLDEN[k] for k in ("seed", "B", "P", "size", "iters"))
INPUT_DIM = GOLDEN["input_dim"]
STEP_LENGTH, STEP_DECAY = 1.0, 1.0   # DeT_DiMP50_Max: box_refinement_step_length = 1, box_refinement_step_decay = 1


class PrRoIPoolStandIn(torch.nn.Module):
    def __init__(self, ph, pw, scale):
        super().__init__()
        self.ph, self.pw, self.scale = ph, pw, scale

    def forward(self, feat, rois):
        return prroi_pool_ref(feat, rois, self.ph, self.pw, self.scale)


def main():
    mgd.install()
    from ltr.models.bbreg.atom_iou_net import AtomIoUNet
    from pytracking.tracker.dimp.dimp import DiMP

    net = AtomIoUNet(input_dim=INPUT_DIM).double().eval()
    sd = synth.make_iounet_state_dict(SEED, input_dim=INPUT_DIM, prefix="")
    net.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    net.prroi_pool3r, net.prroi_pool3t = PrRoIPoolStandIn(3, 3, 1 / 8), PrRoIPoolStandIn(5, 5, 1 / 8)
    net.prroi_pool4r, net.prroi_pool4t = PrRoIPoolStandIn(1, 1, 1 / 16), PrRoIPoolStandIn(3, 3, 1 / 16)
    pre = []   # the hidden layers' pre-activations: the input of each LinearBlock's ReLU
    for blk in (net.fc3_rt, net.fc4_rt):
        blk.relu.register_forward_pre_hook(lambda m, a: pre.append(float(a[0].detach().abs().min() / a[0].detach().abs().max())))
        blk.relu.inplace = False

    x = inputs(SEED, B, P, SIZE, input_dim=INPUT_DIM)
    back = [t.double() for t in x["back"]]
    with torch.no_grad():
        mod = net.get_modulation(back, x["bb"].double())
        feat = net.get_iou_feat(back)
    res = {"seed": np.array(SEED), "mod3": mod[0].numpy(), "mod4": mod[1].numpy(),
           "feat3_ch": feat[0][:, ::16].numpy(), "feat4_ch": feat[1][:, ::16].numpy()}

    boxes = x["boxes"].double()
    bb = boxes.clone().requires_grad_(True)
    iou0 = net.predict_iou(mod, feat, bb)
    iou0.backward(gradient=torch.ones_like(iou0))
    res["iou0"], res["grad0"] = iou0.detach().numpy(), bb.grad.numpy()

    # the reference's loop treats its boxes as one sequence (view(1, -1, 4)): one call per sequence
    stub = types.SimpleNamespace()
    stub.params = types.SimpleNamespace(device="cpu", box_refinement_step_length=STEP_LENGTH,
                                        box_refinement_step_decay=STEP_DECAY, box_refinement_iter=ITERS)
    stub.net = types.SimpleNamespace(bb_regressor=net)
    steps = np.zeros((ITERS, B, P, 4))
    for b in range(B):
        stub.iou_modulation = [m[b:b + 1] for m in mod]
        fb = [f[b:b + 1] for f in feat]
        for it in range(1, ITERS + 1):
            stub.params.box_refinement_iter = it
            out, iou = DiMP.optimize_boxes_default(stub, fb, boxes[b].clone())
            steps[it - 1, b] = out.numpy()
        if b == 0:
            res["iou_final"] = np.zeros((B, P))
        res["iou_final"][b] = iou.numpy()
    res["boxes_steps"] = steps
    res["min_rel_preact"] = np.array(min(pre))
    moved = np.abs(steps[-1] - boxes.numpy()).max()
    np.savez_compressed(os.path.join(HERE, "iounet_det.npz"), **res)
    print(f"wrote iounet_det: iou0 {res['iou0'].min():.4f}..{res['iou0'].max():.4f}, largest move {moved:.2f} px, "
          f"smallest relative |pre-activation| {min(pre):.2e}, "
          f"{os.path.getsize(os.path.join(HERE, 'iounet_det.npz'))} bytes")


if __name__ == "__main__":
    main()
