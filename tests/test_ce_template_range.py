"""CE_TEMPLATE_RANGE on the host side (no GPU): lib.utils.ce_utils.generate_mask_cond against the reference's own
masks (tests/golden/ce_masks.npz, make_golden_ce_range.py), and the binding of every range to the engine config."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from lib.config.vipt import config as vcfg
from lib.utils import ce_utils
from mmtrack_amd import EngineConfig, _lib
from mmtrack_amd.engine import Engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-modal-trakcing-bechmark_amd")


def _cfg(rng, tsz):
    return NS(DATA=NS(TEMPLATE=NS(SIZE=tsz)), MODEL=NS(BACKBONE=NS(STRIDE=16, CE_TEMPLATE_RANGE=rng)))


@pytest.fixture(scope="module")
def masks():
    return np.load(os.path.join(GOLDEN, "ce_masks.npz"))


def test_fixed_ranges_equal_the_reference(masks):
    """ALL -> None; CTR_POINT / CTR_REC -> the reference's bool [bs, Lz]; NotImplementedError where it raises one
    (e.g. CTR_REC at a 14 x 14 template)."""
    seen = set()
    for rng, tsz, kind in masks["table"]:
        tsz = int(tsz)
        seen.add((rng, tsz, kind))
        if kind == "not_implemented":
            with pytest.raises(NotImplementedError):
                ce_utils.generate_mask_cond(_cfg(rng, tsz), 2, "cpu", None)
            continue
        m = ce_utils.generate_mask_cond(_cfg(rng, tsz), 2, "cpu", None)
        if kind == "none":
            assert m is None
        else:
            assert m.dtype == torch.bool and tuple(m.shape) == (2, (tsz // 16) ** 2)
            np.testing.assert_array_equal(m.numpy(), masks[f"{rng}_{tsz}"])
    assert ("CTR_REC", 224, "not_implemented") in seen and ("CTR_REC", 192, "mask") in seen
    assert ("CTR_POINT", 224, "mask") in seen and ("ALL", 128, "none") in seen
    with pytest.raises(NotImplementedError):
        ce_utils.generate_mask_cond(_cfg("NO_SUCH_RANGE", 128), 1, "cpu", None)


@pytest.mark.parametrize("tsz", [128, 192])
def test_gt_box_masks_equal_the_reference(masks, tsz):
    """The template box of an init box (transform_bbox_to_crop) and its GT_BOX mask, for non-square boxes, boxes
    reaching past the crop, fractional coordinates and empty masks (which the helper returns as the reference does)."""
    boxes, tb, rf, ref = masks["gt_boxes"], masks[f"gt_tbox_{tsz}"], masks[f"gt_rf_{tsz}"], masks[f"gt_mask_{tsz}"]
    assert len(boxes) >= 12 and (ref.sum(1) == 0).any() and len(set(ref.sum(1).tolist())) >= 4
    for i, b in enumerate(boxes):
        t = ce_utils.template_box_in_crop([float(v) for v in b], float(rf[i]), tsz)
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, 4)
        np.testing.assert_array_equal(t[0].numpy(), tb[i])
        m = ce_utils.generate_mask_cond(_cfg("GT_BOX", tsz), 1, "cpu", t)
        assert m.dtype == torch.bool
        np.testing.assert_array_equal(m[0].numpy(), ref[i], err_msg=str(b))


def _host_engine(**kw):
    """An Engine object without a device engine behind it: the host-side mask logic alone."""
    e = object.__new__(Engine)
    e.cfg = EngineConfig(**kw)
    return e


def test_engine_masks_follow_the_range(masks):
    boxes, ref = masks["gt_boxes"], masks["gt_mask_128"]
    e = _host_engine(ce_template_range="GT_BOX")
    for b, r in zip(boxes, ref):
        if r.any():
            np.testing.assert_array_equal(e._range_mask([float(v) for v in b]), r)
        else:
            with pytest.raises(ValueError, match="selects no template token"):
                e._range_mask([float(v) for v in b])
    assert e._range_mask([10.0, 10.0, 0.0, 0.0]) is None   # left to the engine's "Too small bounding box."
    assert _host_engine(ce_template_range="ALL")._range_mask([1.0, 2.0, 30.0, 40.0]).all()
    np.testing.assert_array_equal(_host_engine(ce_template_range="CTR_REC")._range_mask([1.0, 2.0, 30.0, 40.0]),
                                  masks["CTR_REC_128"][0])
    assert _host_engine(ce_template_range="MASK")._range_mask([1.0, 2.0, 30.0, 40.0]) is None
    assert _host_engine(ce_template_range="CTR_POINT")._range_mask([1.0, 2.0, 30.0, 40.0]) is None
    with pytest.raises(NotImplementedError):   # where the reference raises: CTR_REC at a 14 x 14 template
        _host_engine(ce_template_range="CTR_REC", template_size=224)._range_mask([1.0, 2.0, 30.0, 40.0])


def test_to_c_accepts_every_range():
    assert _lib.MMT_CE_TEMPLATE_MASK == -2
    assert EngineConfig(ce_template_range="CTR_POINT").to_c().ce_template_index == 27
    for rng in ("ALL", "CTR_REC", "GT_BOX", "MASK"):
        c = EngineConfig(ce_template_range=rng).to_c()
        assert c.ce_template_index == _lib.MMT_CE_TEMPLATE_MASK and c.n_ce == 3
    assert EngineConfig(ce_template_range="ALL", ce_loc=[], ce_keep_ratio=[]).to_c().ce_template_index == -1
    with pytest.raises(ValueError):
        EngineConfig(ce_template_range="CENTER").to_c()


def test_yaml_without_the_key_is_all(tmp_path):
    """The config default is ALL, as the reference's: a yaml that omits CE_TEMPLATE_RANGE builds a mask-mode config."""
    src = open(os.path.join(PKG, "experiments", "vipt", "deep_rgbt.yaml")).read().splitlines()
    kept = [ln for ln in src if "CE_TEMPLATE_RANGE" not in ln]
    assert len(kept) == len(src) - 1
    y = tmp_path / "no_range.yaml"
    y.write_text("\n".join(kept) + "\n")
    vcfg.reset_config()
    try:
        vcfg.update_config_from_file(str(y))
        ec = EngineConfig.from_cfg(vcfg.cfg)
        assert ec.ce_template_range == "ALL" and ec.mask_mode
        assert ec.to_c().ce_template_index == _lib.MMT_CE_TEMPLATE_MASK
        for rng in ("CTR_REC", "GT_BOX"):
            vcfg.cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE = rng
            assert EngineConfig.from_cfg(vcfg.cfg).to_c().ce_template_index == _lib.MMT_CE_TEMPLATE_MASK
    finally:
        vcfg.reset_config()
