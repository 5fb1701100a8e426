"""Candidate elimination over a template mask (CE_TEMPLATE_RANGE = ALL / CTR_REC / GT_BOX, and the engine's MASK
mode) end to end against the reference's goldens (tests/golden/make_golden_ce_range.py) and the CPU oracle, at the
thresholds of test_gpu_parity.test_network_matches_reference_golden: removed sets identical, CE keys < 1e-4 relative,
windowed argmax exact, score / size maps within 1e-3, offsets within 3e-3.  Every recorded reference CE margin is
>= 2.5e-4 relative (asserted by the generator)."""
import math
import os

import numpy as np
import pytest
import torch

from mmtrack_amd import Engine, EngineConfig, synth
from mmtrack_amd.engine import TrackerError
from oracle import crop as ocrop
from oracle import vipt as ov

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SHAPES = {
    "deep_rgbt": dict(kind="vipt", prompt_type="vipt_deep"),
    "ostrack384": dict(kind="ostrack", search_size=384, template_size=192),
}
TAG = {"all": "ALL", "ctrrec": "CTR_REC", "gtbox": "GT_BOX"}


def _cfg(name, rng, **kw):
    base = dict(debug_outputs=True, use_graphs=False, ce_template_range=rng)
    base.update(kw)
    if name == "ostrack384":
        base.update(model="ostrack", prompt_type="none", in_chans=3, template_size=192, search_size=384,
                    search_factor=4.0)
    return EngineConfig(**base)


def identity_frames(zp, xp, search_factor, template_factor=2.0):
    """Frames + box such that sample_target returns zp (initialize) and xp (track) unchanged
    (test_gpu_parity.identity_frames)."""
    T, S = zp.shape[0], xp.shape[0]
    side = T / template_factor
    assert abs(side * search_factor - S) < 1e-9
    cx = cy = 300.0
    box = [cx - side / 2, cy - side / 2, side, side]
    f0 = np.zeros((640, 640, zp.shape[2]), np.uint8)
    f0[int(cy - T / 2):int(cy + T / 2), int(cx - T / 2):int(cx + T / 2)] = zp
    f1 = np.zeros((640, 640, xp.shape[2]), np.uint8)
    f1[int(cy - S / 2):int(cy + S / 2), int(cx - S / 2):int(cx + S / 2)] = xp
    return f0, f1, box


def iou(a, b):
    ax2, ay2, bx2, by2 = a[0] + a[2], a[1] + a[3], b[0] + b[2], b[1] + b[3]
    iw = max(0.0, min(ax2, bx2) - max(a[0], b[0]))
    ih = max(0.0, min(ay2, by2) - max(a[1], b[1]))
    inter = iw * ih
    return inter / (a[2] * a[3] + b[2] * b[3] - inter)


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, rng):
        if (name, rng) not in cache:
            cache[(name, rng)] = Engine(_cfg(name, rng), synth.make_state_dict(0, **SHAPES[name]))
        return cache[(name, rng)]
    yield get
    for e in cache.values():
        e.close()


def check_against_golden(eng, cfg, g, label):
    C = cfg.in_chans
    for j, (sz, ss) in enumerate(g["seeds"]):
        zp = synth.make_patch(int(sz), cfg.template_size, C)
        xp = synth.make_patch(int(ss), cfg.search_size, C)
        f0, f1, box = identity_frames(zp, xp, cfg.search_factor)
        eng.initialize(0, f0, box)
        eng.track(0, f1)
        np.testing.assert_array_equal(eng.debug("crop"), xp)
        maps, res, removed = eng.debug("maps"), eng.debug("result"), eng.debug("removed")
        ref_removed = g[f"removed_{j}"][0]
        assert min(g[f"ce_margin_{j}"]) >= 2.5e-4
        keys, ref_keys = eng.debug("ce_keys"), g[f"ce_keys_{j}"]
        m = ref_keys > 0
        rel = np.abs(keys[m] - ref_keys[m]) / ref_keys[m]
        gs = g[f"score_map_{j}"][0, 0]
        print(f"{label}[{j}] CE score max rel err {rel.max():.2e} (reference min margin {min(g[f'ce_margin_{j}']):.2e}), "
              f"max|dscore| {np.abs(maps[0] - gs).max():.2e}")
        np.testing.assert_array_equal(np.sort(removed[:len(ref_removed)]), np.sort(ref_removed))
        assert rel.max() < 1e-4
        np.testing.assert_allclose(maps[0], gs, atol=1e-3)
        np.testing.assert_allclose(maps[1:3], g[f"size_map_{j}"][0], atol=1e-3)
        np.testing.assert_allclose(maps[3:5], g[f"offset_map_{j}"][0], atol=3e-3)
        assert int(res[5]) == int(g[f"resp_argmax_{j}"][0]), "windowed argmax differs from the reference"
        if f"feat_rows_{j}" in g.files:
            np.testing.assert_allclose(eng.debug("feat")[::8], g[f"feat_rows_{j}"], atol=5e-3)


@pytest.mark.parametrize("name,tag", [("deep_rgbt", "all"), ("deep_rgbt", "ctrrec"), ("deep_rgbt", "gtbox"),
                                      ("ostrack384", "all"), ("ostrack384", "ctrrec")])
def test_network_matches_reference_golden_of_the_range(engines, name, tag):
    """An engine built with the range forms the slot's mask at initialize (GT_BOX: from the init box, the 4 x 4 block
    of the identity frames) and reproduces the reference's outputs under that mask."""
    g = np.load(os.path.join(GOLDEN, f"net_{name}_{tag}.npz"))
    cfg = _cfg(name, TAG[tag])
    eng = engines(name, TAG[tag])
    side = cfg.template_size / 2
    np.testing.assert_array_equal(eng._range_mask([300.0 - side / 2, 300.0 - side / 2, side, side]), g["ce_mask"])
    if tag == "gtbox":
        assert int(g["ce_mask"].sum()) == 16
    check_against_golden(eng, cfg, g, f"{name}/{TAG[tag]}")


def test_ctr_point_golden_through_mask_mode(engines):
    """The committed CTR_POINT golden reproduced by a MASK-mode engine with the single token 27 set: the old
    goldens through the new kernel."""
    cfg = _cfg("deep_rgbt", "MASK")
    eng = engines("deep_rgbt", "MASK")
    mask = np.zeros(64, bool)
    mask[27] = True
    eng.set_ce_template_mask(0, mask)
    check_against_golden(eng, cfg, np.load(os.path.join(GOLDEN, "net_deep_rgbt.npz")), "deep_rgbt/MASK{27}")


def test_random_pairs_under_all_match_the_oracle(engines):
    """Four random crop pairs beyond the goldens under ALL against the fp32 CPU oracle with box_mask_z = None; no
    excused CE flips: the oracle's margins on these pairs are >= 1.1e-3, above 4x the 2e-4 key-error bound."""
    cfg = _cfg("deep_rgbt", "ALL")
    eng = engines("deep_rgbt", "ALL")
    sd = synth.make_state_dict(0, **SHAPES["deep_rgbt"])
    ocfg = ov.NetCfg(ce_template_range="ALL")
    for j in range(4):
        zp = synth.make_patch(900 + j, cfg.template_size, cfg.in_chans)
        xp = synth.make_patch(1900 + j, cfg.search_size, cfg.in_chans)
        f0, f1, box = identity_frames(zp, xp, cfg.search_factor)
        eng.initialize(0, f0, box)
        eng.track(0, f1)
        res, removed, keys = eng.debug("result"), eng.debug("removed"), eng.debug("ce_keys")
        tr = {}
        out = ov.forward(sd, ocrop.preprocess(zp), ocrop.preprocess(xp), ocfg, None, trace=tr)
        kerr = max(float(np.max(np.abs(keys[st][k > 0] - k[k > 0]) / k[k > 0])) for st, k in
                   enumerate(t.numpy() for t in tr["ce_keys"]))
        print(f"ALL random pair {j}: oracle min CE margin {min(tr['ce_margin']):.2e}, key error {kerr:.2e}")
        assert min(tr["ce_margin"]) >= 4 * 2e-4
        assert kerr < 2e-4
        ref_rm = torch.cat(out["removed_indexes_s"], dim=1)[0].numpy()
        np.testing.assert_array_equal(np.sort(removed[:len(ref_rm)]), np.sort(ref_rm))
        resp = (ov.hann2d(ocfg.feat_sz) * out["score_map"]).flatten()
        assert int(res[5]) == int(torch.argmax(resp))
        pb = ov.cal_bbox(resp.view(1, 1, ocfg.feat_sz, ocfg.feat_sz), out["size_map"], out["offset_map"],
                         ocfg.feat_sz)[0].numpy()
        to_xywh = lambda b: [b[0] - b[2] / 2, b[1] - b[3] / 2, b[2], b[3]]
        assert iou(to_xywh(res[:4]), to_xywh(pb)) >= 0.999


def test_tracker_steps_gt_box_match_reference(engines):
    """The reference ViPTTrack with CE_TEMPLATE_RANGE = GT_BOX on a non-square init box (an 18-token mask: two row
    blocks), teacher-forced as test_gpu_parity.test_tracker_steps_match_reference: IoU >= 0.999 and best score
    within 1e-3 on every frame."""
    g = np.load(os.path.join(GOLDEN, "tracker_steps_deep_rgbt_gtbox.npz"))
    seed, n, H, W, C = [int(v) for v in g["meta"]]
    assert (n, H, W) == (8, 480, 640) and g["init_box"][2] != g["init_box"][3]
    assert g["ce_margins"].min() >= 2.5e-4
    frames, _ = synth.make_frames(seed, n, H, W, C, box=tuple(g["init_box"]))
    eng = engines("deep_rgbt", "GT_BOX")
    np.testing.assert_array_equal(eng._range_mask(list(g["init_box"])), g["ce_mask"])
    eng.initialize(0, frames[0], list(g["init_box"]))
    ious, dsc = [], []
    for t in range(1, n):
        eng.set_state(0, g["states"][t])
        box, score = eng.track(0, frames[t])
        ious.append(iou(box, g["boxes"][t]))
        dsc.append(abs(score - g["scores"][t]))
    print("GT_BOX teacher-forced per-step IoU vs reference:", np.round(ious, 5), "max|dscore|", max(dsc))
    assert min(ious) >= 0.999
    assert max(dsc) < 1e-3


def test_gt_box_yaml_through_the_tracker_class():
    """The same golden through the unchanged reference-shaped tracker class: a cfg whose CE_TEMPLATE_RANGE is GT_BOX
    builds an engine (EngineConfig.from_cfg) and ViPTTrack.initialize / track give the reference's boxes."""
    import lib.test.parameter.vipt as vp
    from lib.config.vipt.config import reset_config
    from lib.test.tracker.vipt import ViPTTrack
    g = np.load(os.path.join(GOLDEN, "tracker_steps_deep_rgbt_gtbox.npz"))
    seed, n, H, W, C = [int(v) for v in g["meta"]]
    frames, _ = synth.make_frames(seed, n, H, W, C, box=tuple(g["init_box"]))
    params = vp.parameters("deep_rgbt")
    tr = None
    try:
        params.cfg.MODEL.BACKBONE.CE_TEMPLATE_RANGE = "GT_BOX"
        params.state_dict = synth.make_state_dict(0, **SHAPES["deep_rgbt"])
        tr = ViPTTrack(params)
        assert tr.engine.cfg.ce_template_range == "GT_BOX" and tr.engine.cfg.mask_mode
        tr.initialize(frames[0], {"init_bbox": list(g["init_box"])})
        for t in range(1, 4):
            tr.engine.set_state(0, g["states"][t])
            out = tr.track(frames[t])
            assert iou(out["target_bbox"], g["boxes"][t]) >= 0.999
            assert abs(out["best_score"] - g["scores"][t]) < 1e-3
    finally:
        reset_config()
        if tr is not None:
            tr.engine.close()


def test_mask_api_errors(engines):
    eng = engines("deep_rgbt", "MASK")
    with pytest.raises(ValueError):
        eng.set_ce_template_mask(0, np.zeros(64, bool))          # no token
    with pytest.raises(ValueError):
        eng.set_ce_template_mask(0, np.ones(63, bool))           # n != Lz
    with pytest.raises(ValueError):
        eng.set_ce_template_mask(1, np.ones(64, bool))           # slot >= max_batch
    plain = Engine(EngineConfig(), synth.make_state_dict(0, **SHAPES["deep_rgbt"]))
    try:
        with pytest.raises(TrackerError):                        # not in mask mode: MMT_E_STATE
            plain.set_ce_template_mask(0, np.ones(64, bool))
    finally:
        plain.close()
    gt = engines("deep_rgbt", "GT_BOX")
    with pytest.raises(ValueError, match="selects no template token"):
        gt.initialize(0, np.zeros((480, 640, 6), np.uint8), [0.0, 0.0, 400.0, 1.0])


def _stages(removed):
    """The removed slots of the three CE stages (256 -> 180 -> 126 -> 89), each sorted."""
    out, off, ls = [], 0, 256
    for _ in range(3):
        keep = math.ceil(0.7 * ls)
        out.append(np.sort(removed[off:off + ls - keep]))
        off += ls - keep
        ls = keep
    return np.concatenate(out)


def test_slots_with_different_masks_in_one_graph_launch():
    """max_batch = 3, MASK mode, captured graphs: three slots with different masks and counts in one track_batch give
    the removed sets and argmax of the same sequences tracked alone; a mask set after a replayed frame takes effect in
    the next replay for that slot alone (the kernel reads the lists from fixed device addresses)."""
    sd = synth.make_state_dict(0, **SHAPES["deep_rgbt"])
    seqs = [synth.make_frames(40 + i, 4, 360, 480, 6, box=(200.0 + 10 * i, 150.0, 40.0 + 5 * i, 30.0)) for i in
            range(3)]
    one, rec, r17, full = np.zeros(64, bool), np.zeros((8, 8), bool), np.zeros(64, bool), np.ones(64, bool)
    one[27] = True
    rec[3:5, 3:5] = True
    r17[::3][:17] = True
    masks = [one, rec.reshape(-1), r17]
    eng = Engine(EngineConfig(max_batch=3, debug_outputs=True, use_graphs=True, ce_template_range="MASK"), sd)
    solo = Engine(EngineConfig(max_batch=1, debug_outputs=True, use_graphs=True, ce_template_range="MASK"), sd)
    fresh = None
    try:
        for i, (fr, gt) in enumerate(seqs):
            eng.set_ce_template_mask(i, masks[i])
            eng.initialize(i, fr[0], list(gt[0]))
        got = {}
        for t in (1, 2, 3):   # frame 1 runs eagerly and captures, frames 2 and 3 replay
            if t == 3:
                state1 = eng.state(1)
                eng.set_ce_template_mask(1, full)
            eng.track_batch(0, [seqs[i][0][t] for i in range(3)])
            for i in range(3):
                got[(i, t)] = (_stages(eng.debug("removed", i)), int(eng.debug("result", i)[5]))
        for i, (fr, gt) in enumerate(seqs):
            solo.set_ce_template_mask(0, masks[i])
            solo.initialize(0, fr[0], list(gt[0]))
            for t in (1, 2, 3):
                solo.track(0, fr[t])
                alone = (_stages(solo.debug("removed")), int(solo.debug("result")[5]))
                if i == 1 and t == 3:
                    old = alone   # what slot 1's previous mask would have removed
                    continue
                np.testing.assert_array_equal(got[(i, t)][0], alone[0], err_msg=f"slot {i} frame {t}")
                assert got[(i, t)][1] == alone[1], (i, t)
        fresh = Engine(EngineConfig(max_batch=1, debug_outputs=True, use_graphs=True, ce_template_range="MASK"), sd)
        fresh.set_ce_template_mask(0, full)
        fresh.initialize(0, seqs[1][0][0], list(seqs[1][1][0]))
        fresh.set_state(0, state1)
        fresh.track(0, seqs[1][0][3])
        np.testing.assert_array_equal(got[(1, 3)][0], _stages(fresh.debug("removed")))
        assert got[(1, 3)][1] == int(fresh.debug("result")[5])
        assert not np.array_equal(got[(1, 3)][0], old[0]), "the new mask was meant to change slot 1's removed set"
    finally:
        eng.close()
        solo.close()
        if fresh is not None:
            fresh.close()
