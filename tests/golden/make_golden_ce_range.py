"""Golden fixtures for candidate elimination over a template mask (CE_TEMPLATE_RANGE = ALL / CTR_REC / GT_BOX), from
the REFERENCE itself.  Runs in the build container only, against the reference checkout make_golden.py names and
with its shims and helpers; writes

* net_deep_rgbt_{all,ctrrec,gtbox}.npz, net_ostrack384_{all,ctrrec}.npz   (the key format of make_golden.net_fixture;
  plus ce_mask, the reference's box_mask_z, all-True for ALL);
* tracker_steps_deep_rgbt_gtbox.npz   (the reference ViPTTrack with GT_BOX, teacher-forced, non-square init box);
* ce_masks.npz   (generate_mask_cond's masks for every (range, template feature size) it supports, the sizes where it
  raises NotImplementedError, and GT_BOX masks of a dozen init boxes with the template boxes they came from).

Every CE boundary margin recorded here must be >= 2.5e-4 relative, the floor of the committed goldens
(test_gpu_parity.py); the generator fails otherwise, so a seed is never accepted by what the engine makes of it.

Usage:  python tests/golden/make_golden_ce_range.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MARGIN_FLOOR = 2.5e-4
DEEP_SEEDS = [(101, 201), (102, 202), (113, 213), (114, 214)]
OSTRACK_SEEDS = [(141, 241), (144, 244), (145, 245)]
RANGE_TAG = {"ALL": "all", "CTR_REC": "ctrrec", "GT_BOX": "gtbox"}
# init boxes (x, y, w, h, frame pixels) for the GT_BOX masks: square, non-square, elongated past the crop on either
# axis (negative slice bounds), fractional, tiny, and boxes whose rasterised block misses every token's sample rows
# or is an empty slice (empty masks)
GT_BOXES = [(268.0, 268.0, 64.0, 64.0), (300.0, 200.0, 40.0, 30.0), (280.0, 190.0, 56.0, 30.0),
            (220.0, 140.0, 52.0, 44.0), (100.0, 100.0, 200.0, 10.0), (100.0, 100.0, 12.0, 180.0),
            (10.25, 20.75, 7.5, 13.5), (33.3, 47.9, 81.7, 19.1), (5.0, 5.0, 3.0, 2.0), (150.5, 90.5, 25.0, 100.0),
            (60.0, 40.0, 90.0, 35.5), (0.0, 0.0, 400.0, 1.0)]


def reference_template_box(init_box, template_factor, template_size):
    """ViPTTrack.initialize's template_bbox (vipt.py:43-54) without the image: resize_factor as sample_target forms it."""
    import math
    from lib.train.data.processing_utils import transform_image_to_crop
    x, y, w, h = init_box
    crop_sz = math.ceil(math.sqrt(w * h) * template_factor)
    rf = template_size / crop_sz
    box = torch.tensor(list(init_box))
    tb = transform_image_to_crop(box, box, rf, torch.Tensor([template_size, template_size]), normalize=True)
    return tb.view(1, 4), rf


def with_range(cfg, rng):
    cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE = rng
    return cfg


def check_margins(path, keys):
    g = np.load(path)
    lo = min(float(np.min(g[k])) for k in keys(g))
    assert lo >= MARGIN_FLOOR, f"{path}: CE boundary margin {lo:.2e} below the floor {MARGIN_FLOOR:.1e}"
    return lo


def net_fixtures(build, cfg_of, sd, name, C, tsz, ssz, seeds, ranges):
    from lib.utils.ce_utils import generate_mask_cond
    for rng in ranges:
        cfg = with_range(cfg_of(), rng)
        model = build(cfg, training=False).eval()
        model.load_state_dict(sd, strict=True)
        gt = None
        if rng == "GT_BOX":   # the identity-frame template box of test_gpu_parity.identity_frames
            side = tsz / cfg.TEST.TEMPLATE_FACTOR
            gt, rf = reference_template_box((300.0 - side / 2, 300.0 - side / 2, side, side), cfg.TEST.TEMPLATE_FACTOR, tsz)
            assert rf == 1.0
        mask = generate_mask_cond(cfg, 1, "cpu", gt)

        def run_net(model, cfg, z, x, C, mask=mask):
            with torch.no_grad():
                return model.forward(template=z, search=x, ce_template_mask=mask)
        mg.run_net = run_net
        full = f"{name}_{RANGE_TAG[rng]}"
        mg.net_fixture(full, model, cfg, sd, C, tsz, ssz, seeds, feat_seeds=1)
        path = os.path.join(HERE, f"net_{full}.npz")
        lo = check_margins(path, lambda g: [k for k in g.files if k.startswith("ce_margin_")])
        g = dict(np.load(path))
        lz = (tsz // 16) ** 2
        g["ce_mask"] = np.ones(lz, bool) if mask is None else mask[0].numpy()
        np.savez_compressed(path, **g)
        print(f"  {full}: mask of {int(g['ce_mask'].sum())} tokens, min CE margin {lo:.2e}, {os.path.getsize(path)} bytes")


def tracker_fixture():
    """The reference ViPTTrack with GT_BOX on a non-square init box, teacher-forced, 8 frames of 640 x 480: the first
    of the candidate sequence seeds whose 21 reference CE margins all meet the floor (61 has one of 1.5e-5)."""
    orig = mg.load_cfg
    mg.load_cfg = lambda y: with_range(orig(y), "GT_BOX")
    sd = mg.synth.make_state_dict(0, kind="vipt", prompt_type="vipt_deep")
    init_box = (280.0, 190.0, 56.0, 30.0)
    try:
        for seed in (61, 62, 63, 64, 65):
            mg.CE_LOG.clear()
            mg.tracker_fixture("deep_rgbt_gtbox", "deep_rgbt", sd, 8, seed, 480, 640, 6, init_box, steps=True)
            margins = np.array([m for _, _, m in mg.CE_LOG])
            assert len(margins) == 7 * 3
            if margins.min() >= MARGIN_FLOOR:
                break
            print(f"  sequence seed {seed}: min reference CE margin {margins.min():.2e} below the floor, not used")
    finally:
        mg.load_cfg = orig
    path = os.path.join(HERE, "tracker_steps_deep_rgbt_gtbox.npz")
    if margins.min() < MARGIN_FLOOR:
        os.remove(path)
        raise AssertionError("no candidate sequence meets the CE margin floor")
    g = dict(np.load(path))
    g["ce_margins"] = margins
    g["ce_mask"] = template_masks_of([init_box], 128, 2.0)[2][0]
    np.savez_compressed(path, **g)
    print(f"  tracker_steps_deep_rgbt_gtbox: seed {seed}, mask of {int(g['ce_mask'].sum())} tokens, min CE margin "
          f"{margins.min():.2e}")


def template_masks_of(boxes, template_size, template_factor):
    from lib.utils.ce_utils import generate_mask_cond
    cfg = with_range(mg.load_cfg("deep_rgbt"), "GT_BOX")
    cfg.DATA.TEMPLATE.SIZE = template_size
    tbs, rfs, masks = [], [], []
    for b in boxes:
        tb, rf = reference_template_box(b, template_factor, template_size)
        tbs.append(tb[0].numpy())
        rfs.append(rf)
        masks.append(generate_mask_cond(cfg, 1, "cpu", tb)[0].numpy())
    return np.array(tbs), np.array(rfs), np.array(masks)


def masks_fixture():
    from lib.utils.ce_utils import generate_mask_cond
    res = {}
    table = []   # (range, template size, "mask" | "none" | "not_implemented")
    for rng in ("ALL", "CTR_POINT", "CTR_REC"):
        for tsz in (112, 128, 192, 224, 256):
            cfg = with_range(mg.load_cfg("deep_rgbt"), rng)
            cfg.DATA.TEMPLATE.SIZE = tsz
            try:
                m = generate_mask_cond(cfg, 2, "cpu", None)
            except NotImplementedError:
                table.append((rng, str(tsz), "not_implemented"))
                continue
            table.append((rng, str(tsz), "none" if m is None else "mask"))
            if m is not None:
                assert m.shape == (2, (tsz // 16) ** 2) and m.dtype == torch.bool
                res[f"{rng}_{tsz}"] = m.numpy()
    res["table"] = np.array(table)
    res["gt_boxes"] = np.array(GT_BOXES)
    for tsz in (128, 192):
        tbs, rfs, masks = template_masks_of(GT_BOXES, tsz, 2.0)
        res[f"gt_tbox_{tsz}"], res[f"gt_rf_{tsz}"], res[f"gt_mask_{tsz}"] = tbs, rfs, masks
        print(f"  GT_BOX masks at {tsz}: tokens per box {masks.sum(1).tolist()}")
        # (a box a little wider than its crop has a negative left bound of -1, which as a Python slice starts at the
        # last column: an empty mask too)
        assert (masks.sum(1) == 0).sum() >= 1, "at least the last box is meant to give an empty mask"
    np.savez_compressed(os.path.join(HERE, "ce_masks.npz"), **res)
    print("wrote ce_masks", table)


def main():
    mg.install_shims()
    sys.path.insert(0, os.path.join(mg.REF, "ViPT"))
    torch.set_num_threads(8)
    from lib.models.vipt import build_ostrack, build_viptrack
    mg.install_ce_recorder()
    if "--tracker" in sys.argv:   # the tracker sequence alone
        tracker_fixture()
        return
    masks_fixture()
    net_fixtures(build_viptrack, lambda: mg.load_cfg("deep_rgbt"), mg.synth.make_state_dict(0, kind="vipt", prompt_type="vipt_deep"),
                 "deep_rgbt", 6, 128, 256, DEEP_SEEDS, ("ALL", "CTR_REC", "GT_BOX"))
    net_fixtures(build_ostrack, mg.ostrack_cfg, mg.synth.make_state_dict(0, kind="ostrack", search_size=384, template_size=192),
                 "ostrack384", 3, 192, 384, OSTRACK_SEEDS, ("ALL", "CTR_REC"))
    tracker_fixture()


if __name__ == "__main__":
    main()
