"""End-to-end parity of the HIP engine against the reference's golden outputs and the CPU oracle.

Network-level: the golden fixtures (tests/golden/net_*.npz, produced by the reference itself)
were computed on pre-cropped template/search patches.  The engine only takes frames, so each
patch is placed in a canvas where the tracker's own crop is an exact identity (box 64x64 ->
template crop 128 = output size, search crop 256 = output size; the resize at scale 1 reproduces
the input bit for bit, see test_oracle_golden.py).  Tolerances (bf16 GEMM operands, fp32
accumulation, fp32 residual / LayerNorm / softmax / CE scores):

parity mode (precision "fp32", f16x3 products -- the default):
* CE kept sets identical to the reference's (its recorded boundary margins are >= 2.5e-4 relative; the
  engine's CE scores agree to < 1e-4 relative);
* argmax of the Hann-windowed score map: exact;
* score / size maps |d| <= 1e-3, offset maps <= 3e-3;
* predicted boxes: IoU >= 0.999 against the reference (tracker sequences and random pairs).
The bf16 mode is checked only with teacher-forced CE (its arithmetic error, not parity).
"""
import os

import numpy as np
import pytest
import torch

from mmtrack_amd import Engine, EngineConfig, synth
from mmtrack_amd.engine import TrackerError
from oracle import crop as ocrop
from oracle import tracker as otracker
from oracle import vipt as ov

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

def _cfg(name, **kw):
    base = dict(debug_outputs=True, use_graphs=False)
    base.update(kw)
    if name == "shaw_rgbt":
        base.setdefault("prompt_type", "vipt_shaw")
    if name == "ostrack384":
        base.update(model="ostrack", prompt_type="none", in_chans=3, template_size=192, search_size=384,
                    search_factor=4.0)
    return EngineConfig(**base)


SHAPES = {
    "deep_rgbt": dict(kind="vipt", prompt_type="vipt_deep"),
    "deep_rgbd": dict(kind="vipt", prompt_type="vipt_deep"),
    "shaw_rgbt": dict(kind="vipt", prompt_type="vipt_shaw"),
    "ostrack384": dict(kind="ostrack", search_size=384, template_size=192),
}
NETS = {name: (SHAPES[name], _cfg(name)) for name in SHAPES}


def identity_frames(zp, xp, search_factor, template_factor=2.0):
    """Frames + box such that sample_target returns zp (initialize) and xp (track) unchanged."""
    T, S = zp.shape[0], xp.shape[0]
    side = T / template_factor           # template crop = sqrt(w*h) * factor = T
    assert abs(side * search_factor - S) < 1e-9
    cx = cy = 300.0
    box = [cx - side / 2, cy - side / 2, side, side]
    H = W = 640
    f0 = np.zeros((H, W, zp.shape[2]), np.uint8)
    f0[int(cy - T / 2):int(cy + T / 2), int(cx - T / 2):int(cx + T / 2)] = zp
    f1 = np.zeros((H, W, xp.shape[2]), np.uint8)
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

    def get(name, precision="fp32"):
        key = (name, precision)
        if key not in cache:
            cache[key] = Engine(_cfg(name, precision=precision), synth.make_state_dict(0, **SHAPES[name]))
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


@pytest.mark.parametrize("name", list(NETS))
def test_network_matches_reference_golden(engines, name):
    """fp32-faithful mode: the reference's own outputs, CE decisions identical, argmax exact."""
    cfg = _cfg(name)
    eng = engines(name, "fp32")
    g = np.load(os.path.join(GOLDEN, f"net_{name}.npz"))
    C = cfg.in_chans
    for j, (sz, ss) in enumerate(g["seeds"]):
        zp = synth.make_patch(int(sz), cfg.template_size, C)
        xp = synth.make_patch(int(ss), cfg.search_size, C)
        f0, f1, box = identity_frames(zp, xp, cfg.search_factor)
        eng.initialize(0, f0, box)
        eng.track(0, f1)
        np.testing.assert_array_equal(eng.debug("crop"), xp)   # the crop really is the identity
        maps = eng.debug("maps")
        res = eng.debug("result")
        removed = eng.debug("removed")
        ref_removed = g[f"removed_{j}"][0]
        # every recorded reference CE margin is >= 2.5e-4 relative, far above the split products' error
        assert min(g[f"ce_margin_{j}"]) > 1e-5
        np.testing.assert_array_equal(np.sort(removed[:len(ref_removed)]), np.sort(ref_removed))
        keys = eng.debug("ce_keys")
        ref_keys = g[f"ce_keys_{j}"]
        m = ref_keys > 0
        rel = np.abs(keys[m] - ref_keys[m]) / ref_keys[m]
        print(f"{name}[{j}] CE score max rel err {rel.max():.2e} (reference min margin {min(g[f'ce_margin_{j}']):.2e})")
        assert rel.max() < 1e-4
        gs = g[f"score_map_{j}"][0, 0]
        print(f"{name}[{j}] fp32-faithful max|dscore| {np.abs(maps[0] - gs).max():.2e}")
        np.testing.assert_allclose(maps[0], gs, atol=1e-3)
        np.testing.assert_allclose(maps[1:3], g[f"size_map_{j}"][0], atol=1e-3)
        np.testing.assert_allclose(maps[3:5], g[f"offset_map_{j}"][0], atol=3e-3)
        assert int(res[5]) == int(g[f"resp_argmax_{j}"][0]), "windowed argmax differs from the reference"
        if f"feat_rows_{j}" in g.files:
            feat = eng.debug("feat")
            np.testing.assert_allclose(feat[::8], g[f"feat_rows_{j}"], atol=5e-3)


@pytest.mark.parametrize("name,n", [("deep_rgbt", 24), ("deep_rgbd", 12), ("shaw_rgbt", 12), ("ostrack384", 12)])
def test_parity_random_pairs(engines, name, n):
    """The default (parity) mode against the fp32 CPU oracle on random crop pairs beyond the goldens, at the
    north star's thresholds: CE kept sets identical, windowed argmax identical, box IoU >= 0.999.  A CE
    flip is excused only where the reference's own boundary margin is below 4x the measured CE-score error
    of that pair (fp32 noise of both sides); none of these pairs comes near that."""
    cfg = _cfg(name)
    eng = engines(name, "fp32")
    sd = synth.make_state_dict(0, **SHAPES[name])
    ocfg = ov.NetCfg(kind=SHAPES[name]["kind"], prompt_type=SHAPES[name].get("prompt_type", "vipt_deep"),
                     search_size=cfg.search_size, template_size=cfg.template_size)
    Lx = ocfg.lens_x
    for j in range(n):
        zp = synth.make_patch(900 + j, cfg.template_size, cfg.in_chans)
        xp = synth.make_patch(1900 + j, cfg.search_size, cfg.in_chans)
        f0, f1, box = identity_frames(zp, xp, cfg.search_factor)
        eng.initialize(0, f0, box)
        eng.track(0, f1)
        res, removed, keys = eng.debug("result"), eng.debug("removed"), eng.debug("ce_keys")
        tr = {}
        out = ov.forward(sd, ocrop.preprocess(zp), ocrop.preprocess(xp), ocfg, ov.ce_template_mask(ocfg), trace=tr)
        kerr = max(float(np.max(np.abs(keys[st][k > 0] - k[k > 0]) / k[k > 0])) for st, k in
                   enumerate(t.numpy() for t in tr["ce_keys"]))
        if min(tr["ce_margin"]) > 4 * kerr:
            ref_rm = torch.cat(out["removed_indexes_s"], dim=1)[0].numpy()
            np.testing.assert_array_equal(np.sort(removed[:len(ref_rm)]), np.sort(ref_rm))
            resp = (ov.hann2d(ocfg.feat_sz) * out["score_map"]).flatten()
            assert int(res[5]) == int(torch.argmax(resp)), (name, j)
            pb = ov.cal_bbox(resp.view(1, 1, ocfg.feat_sz, ocfg.feat_sz), out["size_map"], out["offset_map"],
                             ocfg.feat_sz)[0].numpy()
            to_xywh = lambda b: [b[0] - b[2] / 2, b[1] - b[3] / 2, b[2], b[3]]
            assert iou(to_xywh(res[:4]), to_xywh(pb)) >= 0.999
        else:
            print(f"{name}[{j}]: reference CE margin {min(tr['ce_margin']):.2e} within 4x the score error {kerr:.2e}")
        assert kerr < 2e-4, kerr
        assert Lx == keys.shape[1]


def test_bf16_mode_teacher_forced(engines):
    """The opt-in bf16 mode is not a parity mode (its CE decisions flip against the
    reference).  With the reference's CE decisions injected (mmt_debug_force_ce) what remains is the bf16
    arithmetic itself: score maps within 3e-2 of the golden, the kept sets the forced ones."""
    eng = engines("deep_rgbt", "bf16")
    cfg = _cfg("deep_rgbt")
    g = np.load(os.path.join(GOLDEN, "net_deep_rgbt.npz"))
    for j, (sz, ss) in enumerate(g["seeds"]):
        zp = synth.make_patch(int(sz), cfg.template_size, cfg.in_chans)
        xp = synth.make_patch(int(ss), cfg.search_size, cfg.in_chans)
        f0, f1, box = identity_frames(zp, xp, cfg.search_factor)
        eng.force_ce(0, g[f"ce_keys_{j}"])
        eng.initialize(0, f0, box)
        eng.track(0, f1)
        eng.force_ce(0, None)
        ref_removed = g[f"removed_{j}"][0]
        np.testing.assert_array_equal(np.sort(eng.debug("removed")[:len(ref_removed)]), np.sort(ref_removed))
        d = np.abs(eng.debug("maps")[0] - g[f"score_map_{j}"][0, 0]).max()
        print(f"bf16 teacher-forced [{j}] score max|d| {d:.3e}")
        assert d < 3e-2


def spans_frame(box, H, W, tol=0.5):
    """A box touching two opposite frame edges (the free-running random-weight trackers grow their boxes until
    clip_box pins them to the frame): an IoU check on it says little, so such frames are held to a looser IoU and
    the set of them is asserted exactly (SPANNING), so a change in which frames saturate does not pass unseen."""
    x, y, w, h = box
    return (x <= tol and x + w >= W - tol) or (y <= tol and y + h >= H - tol)


# the frames of each free-running golden whose reference box spans the frame (fixed by the committed goldens)
SPANNING = {"tracker_deep_rgbt": [], "tracker_deep_rgbd": [10], "tracker_ostrack384": [9, 10, 11]}


@pytest.mark.parametrize("seq", ["deep_rgbt", "deep_rgbd"])
def test_tracker_sequence_matches_reference(engines, seq):
    """Free-running sequences of the reference ViPTTrack (golden: 10 frames 640x480, 20 frames 640x360) vs the
    engine: IoU >= 0.999 on every frame whose reference box does not span the frame (those are listed)."""
    g = np.load(os.path.join(GOLDEN, f"tracker_{seq}.npz"))
    seed, n, H, W, C = [int(v) for v in g["meta"]]
    frames, _ = synth.make_frames(seed, n, H, W, C, box=tuple(g["init_box"]))
    eng = engines("deep_rgbt", "fp32")
    eng.initialize(0, frames[0], list(g["init_box"]))
    ious, spanning = [], []
    for t in range(1, n):
        box, score = eng.track(0, frames[t])
        if spans_frame(g["boxes"][t], H, W):
            spanning.append((t, round(iou(box, g["boxes"][t]), 5)))
        else:
            ious.append(iou(box, g["boxes"][t]))
    print("per-frame IoU vs reference:", np.round(ious, 5), "frame-spanning (IoU >= 0.99):", spanning)
    assert [t for t, _ in spanning] == SPANNING[f"tracker_{seq}"]
    assert len(ious) == n - 1 - len(spanning) and min(ious) >= 0.999
    assert all(v >= 0.99 for _, v in spanning)


@pytest.mark.parametrize("seq", ["deep_rgbt", "deep_rgbd", "ostrack384"])
def test_tracker_steps_match_reference(engines, seq):
    """Teacher-forced one-step checks (tracker_steps_<seq>.npz, make_golden.py --steps): before frame t the
    reference ViPTTrack's state was set to the ground-truth box of frame t - 1, so every frame's crop holds the
    target and no frame saturates; the engine, given the same state through set_state (vipt.py:84-88, 112-118),
    gives the reference's box (IoU >= 0.999) and best score (within 1e-3) on every frame."""
    g = np.load(os.path.join(GOLDEN, f"tracker_steps_{seq}.npz"))
    seed, n, H, W, C = [int(v) for v in g["meta"]]
    frames, _ = synth.make_frames(seed, n, H, W, C, box=tuple(g["init_box"]))
    if seq == "ostrack384":
        cfg = EngineConfig(model="ostrack", prompt_type="none", in_chans=3, template_size=192, search_size=384,
                           search_factor=float(g["search_factor"][0]))
        eng = Engine(cfg, synth.make_state_dict(0, **SHAPES["ostrack384"]))
    else:
        eng = engines("deep_rgbt", "fp32")
    try:
        eng.initialize(0, frames[0], list(g["init_box"]))
        ious, dsc = [], []
        for t in range(1, n):
            assert not spans_frame(g["boxes"][t], H, W)
            eng.set_state(0, g["states"][t])
            box, score = eng.track(0, frames[t])
            ious.append(iou(box, g["boxes"][t]))
            dsc.append(abs(score - g["scores"][t]))
        print(f"{seq} teacher-forced per-step IoU vs reference:", np.round(ious, 5), "max|dscore|", max(dsc))
        assert min(ious) >= 0.999
        assert max(dsc) < 1e-3
    finally:
        if seq == "ostrack384":
            eng.close()


def test_crop_kernel_bit_exact_vs_oracle(engines):
    """A1: GPU sample_target + cv2-INTER_LINEAR restatement == oracle, incl. padding and 2x-area cases."""
    eng = engines("deep_rgbt")
    rng = np.random.Generator(np.random.PCG64(5))
    frame = rng.integers(0, 256, size=(360, 640, 6), dtype=np.uint8)
    cases = [[300.0, 200.0, 40.0, 30.0], [0.0, 0.0, 50.0, 40.0], [600.0, 330.0, 35.0, 25.0],
             [100.5, 50.25, 64.0, 64.0], [200.0, 100.0, 128.0, 128.0], [10.0, 300.0, 12.0, 9.0],
             [250.0, 120.0, 160.0, 90.0]]
    for box in cases:
        eng.initialize(0, frame, [300.0, 200.0, 40.0, 30.0])
        eng.set_state(0, box)
        eng.track(0, frame)
        ref, _ = ocrop.sample_target(frame, box, 4.0, 256)
        np.testing.assert_array_equal(eng.debug("crop"), ref, err_msg=str(box))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_batch_equals_single(engines, precision):
    """track_batch over N sequences (graph-captured) == N independent single-sequence tracks (parity mode: to
    fp32 rounding, one sequence alone runs its few-tile GEMMs split-K, which changes the summation order)."""
    cfg = EngineConfig(max_batch=3, debug_outputs=True, use_graphs=True, precision=precision)
    eng = Engine(cfg, synth.make_state_dict(0, **SHAPES["deep_rgbt"]))
    single = engines("deep_rgbt", precision)
    seqs = [synth.make_frames(40 + i, 4, 360, 480, 6, box=(200.0 + 10 * i, 150.0, 40.0 + 5 * i, 30.0)) for i in
            range(3)]
    for i, (fr, gt) in enumerate(seqs):
        eng.initialize(i, fr[0], list(gt[0]))
    outs_b = []
    for t in range(1, 4):
        boxes, scores = eng.track_batch(0, [seqs[i][0][t] for i in range(3)])
        outs_b.append(boxes)
    for i, (fr, gt) in enumerate(seqs):
        single.initialize(0, fr[0], list(gt[0]))
        for t in range(1, 4):
            box, _ = single.track(0, fr[t])
            if precision == "bf16":   # no split-K in bf16 mode: batch-size independent bit for bit
                np.testing.assert_allclose(outs_b[t - 1][i], box, rtol=1e-6, atol=1e-4)
            else:
                np.testing.assert_allclose(outs_b[t - 1][i], box, rtol=1e-5, atol=1e-3)
    eng.close()


def test_engine_vs_oracle_tracker(engines):
    """Same frames through the CPU oracle tracker and the engine: box IoU per frame."""
    frames, gts = synth.make_frames(77, 8, 480, 640, 6)
    sd = synth.make_state_dict(0, kind="vipt", prompt_type="vipt_deep")
    boxes_o, _ = otracker.run_sequence(otracker.OracleTracker(sd, ov.NetCfg()), frames, gts[0])
    eng = engines("deep_rgbt", "fp32")
    eng.initialize(0, frames[0], list(gts[0]))
    ious = [iou(eng.track(0, frames[t])[0], boxes_o[t]) for t in range(1, 8)]
    print("engine vs oracle IoU:", np.round(ious, 5))
    assert min(ious) >= 0.999


def test_errors_are_reference_shaped(engines):
    eng = engines("deep_rgbt")
    frame = np.zeros((100, 100, 6), np.uint8)
    with pytest.raises(Exception, match="Too small bounding box."):
        eng.initialize(0, frame, [10.0, 10.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        eng.initialize(0, np.zeros((100, 100, 3), np.uint8), [10.0, 10.0, 20.0, 20.0])


def test_device_resident_frames(engines):
    """Frames already in HBM (torch uint8 tensors) give the same result as host frames."""
    eng = engines("deep_rgbt")
    frames, gts = synth.make_frames(12, 3, 480, 640, 6)
    eng.initialize(0, frames[0], list(gts[0]))
    host = [eng.track(0, frames[t])[0] for t in (1, 2)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    eng.initialize(0, dev[0], list(gts[0]))
    devb = [eng.track(0, dev[t])[0] for t in (1, 2)]
    np.testing.assert_allclose(host, devb, rtol=0, atol=0)


@pytest.mark.parametrize("use_graphs", [False, True])
def test_pipelined_frames_equal_blocking(use_graphs):
    """Frames submitted ahead of their fetch (device-resident tracker state: crop geometry and the box
    back-map run on the GPU) give bit-identical boxes and scores to blocking per-frame calls; the host
    copy of the state follows the fetches; tickets are checked."""
    sd = synth.make_state_dict(0, **SHAPES["deep_rgbt"])
    seqs = [synth.make_frames(90 + i, 6, 360, 480, 6, box=(120.0 + 30 * i, 100.0, 36.0 + 4 * i, 28.0)) for i in
            range(3)]
    res = {}
    for mode in ("sync", "pipe"):
        eng = Engine(EngineConfig(max_batch=3, use_graphs=use_graphs), sd)
        for i, (fr, gt) in enumerate(seqs):
            eng.initialize(i, fr[0], list(gt[0]))
        out = []
        if mode == "sync":
            for t in range(1, 6):
                out.append(eng.track_batch(0, [seqs[i][0][t] for i in range(3)]))
        else:
            tickets = [eng.track_batch_submit(0, [seqs[i][0][t] for i in range(3)]) for t in range(1, 4)]
            with pytest.raises(TrackerError):                    # initialize needs nothing in flight
                eng.initialize(0, seqs[0][0][0], list(seqs[0][1][0]))
            out.append(eng.track_batch_fetch(tickets[0]))
            tickets.append(eng.track_batch_submit(0, [seqs[i][0][4] for i in range(3)]))
            for tk in tickets[1:]:
                out.append(eng.track_batch_fetch(tk))
            with pytest.raises(ValueError):                      # already fetched
                eng.track_batch_fetch(tickets[0])
            out.append(eng.track_batch(0, [seqs[i][0][5] for i in range(3)]))
        res[mode] = (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
                     np.array([eng.state(i) for i in range(3)]))
        eng.close()
    for a, b in zip(res["sync"], res["pipe"]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res["pipe"][2], res["pipe"][0][-1])


@pytest.mark.parametrize("nparts", ["2", "4"])
def test_split_launch_equals_single(nparts, monkeypatch):
    """A launch of >= 32 sequences runs as parts on separate HIP streams (engine_forward.cpp enqueue_split, captured
    into one graph); every sequence's boxes equal that sequence tracked alone (to fp32 rounding: the parts'
    few-tile GEMMs may split K differently from a one-sequence launch)."""
    monkeypatch.setenv("MMT_NPARTS", nparts)
    n = 32
    cfg = EngineConfig(max_batch=n, use_graphs=True, precision="fp32")
    sd = synth.make_state_dict(0, **SHAPES["deep_rgbt"])
    eng = Engine(cfg, sd)
    seqs = [synth.make_frames(300 + i, 3, 360, 480, 6, box=(120.0 + 9 * i, 100.0 + 3 * i, 40.0, 32.0))
            for i in range(n)]
    for i, (fr, gt) in enumerate(seqs):
        eng.initialize(i, fr[0], list(gt[0]))
    outs = [eng.track_batch(0, [seqs[i][0][t] for i in range(n)])[0] for t in (1, 2)]
    eng.close()
    single = Engine(EngineConfig(max_batch=1, use_graphs=True, precision="fp32"), sd)
    for i in (0, n // 2 - 1, n // 2, n - 1):
        fr, gt = seqs[i]
        single.initialize(0, fr[0], list(gt[0]))
        for t in (1, 2):
            box, _ = single.track(0, fr[t])
            np.testing.assert_allclose(outs[t - 1][i], box, rtol=1e-5, atol=1e-3)
    single.close()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_split_launch_buffer_views(engines, precision, monkeypatch):
    """A launch whose parts see the activation buffers at a slot b0 != launch row r0 > 0: slots 1..3 of a four-slot
    engine tracked as parts (b0=1, r0=0, n=1) and (b0=2, r0=1, n=2), once eagerly and once as a captured graph, with
    and without the low halves, debug buffers on.  Per sequence: the crop byte for byte, the removed set, boxes
    (test_batch_equals_single's tolerances) and scores (1e-3) of that sequence tracked alone."""
    monkeypatch.setenv("MMT_OVERLAP_MIN", "2")
    monkeypatch.setenv("MMT_NPARTS", "2")
    eng = Engine(EngineConfig(max_batch=4, debug_outputs=True, use_graphs=True, precision=precision),
                 synth.make_state_dict(0, **SHAPES["deep_rgbt"]))
    single = engines("deep_rgbt", precision)
    seqs = [synth.make_frames(60 + k, 3, 360, 480, 6, box=(180.0 + 15 * k, 140.0 + 5 * k, 38.0 + 6 * k, 30.0))
            for k in range(3)]
    for k, (fr, gt) in enumerate(seqs):
        eng.initialize(k + 1, fr[0], list(gt[0]))
    outs, crops, removed = [], None, None
    for t in (1, 2):
        outs.append(eng.track_batch(1, [seqs[k][0][t] for k in range(3)]))
        if t == 1:
            crops = [eng.debug("crop", k) for k in range(3)]
            removed = [np.sort(eng.debug("removed", k)) for k in range(3)]
    eng.close()
    rtol, atol = (1e-6, 1e-4) if precision == "bf16" else (1e-5, 1e-3)
    for k, (fr, gt) in enumerate(seqs):
        single.initialize(0, fr[0], list(gt[0]))
        for t in (1, 2):
            box, score = single.track(0, fr[t])
            if t == 1:
                np.testing.assert_array_equal(crops[k], single.debug("crop"), err_msg=f"crop of sequence {k}")
                np.testing.assert_array_equal(removed[k], np.sort(single.debug("removed")),
                                              err_msg=f"removed set of sequence {k}")
            np.testing.assert_allclose(outs[t - 1][0][k], box, rtol=rtol, atol=atol, err_msg=f"sequence {k} frame {t}")
            assert abs(float(outs[t - 1][1][k]) - float(score)) <= 1e-3, (k, t)


def test_ostrack384_tracker_sequence_matches_reference():
    """C4 at its bench search factor 5.0: the reference build_ostrack network driven by the reference ViPTTrack
    state machine (tracker_ostrack384.npz, make_golden.py ostrack_tracker_fixture; the reference's own OSTrack
    tracker does not run as shipped) against the engine's OSTrack-384 path, 12 frames of 640 x 480 RGB: boxes
    IoU >= 0.999 on every frame, best scores within 1e-3."""
    g = np.load(os.path.join(GOLDEN, "tracker_ostrack384.npz"))
    seed, n, H, W, C = [int(v) for v in g["meta"]]
    assert float(g["search_factor"][0]) == 5.0
    frames, _ = synth.make_frames(seed, n, H, W, C, box=tuple(g["init_box"]))
    cfg = EngineConfig(model="ostrack", prompt_type="none", in_chans=3, template_size=192, search_size=384,
                       search_factor=5.0)
    eng = Engine(cfg, synth.make_state_dict(0, **SHAPES["ostrack384"]))
    try:
        eng.initialize(0, frames[0], list(g["init_box"]))
        ious, dsc, spanning = [], [], []
        for t in range(1, n):
            box, score = eng.track(0, frames[t])
            if spans_frame(g["boxes"][t], H, W):
                spanning.append((t, round(iou(box, g["boxes"][t]), 5)))
                continue
            ious.append(iou(box, g["boxes"][t]))
            dsc.append(abs(score - g["scores"][t]))
        print("OSTrack-384 per-frame IoU vs reference:", np.round(ious, 5), "max|dscore|", max(dsc),
              "frame-spanning (IoU >= 0.99):", spanning)
        assert [t for t, _ in spanning] == SPANNING["tracker_ostrack384"]
        assert len(ious) == n - 1 - len(spanning) and min(ious) >= 0.999
        assert all(v >= 0.99 for _, v in spanning)
        assert max(dsc) < 1e-3
    finally:
        eng.close()
