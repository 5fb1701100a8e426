"""The IoU-Net predictor's host side, without a GPU: the module's import and CPU behaviour, the dimension checks, the
workspace sizes and the K split they imply, the argument checks of every mmt_iounet_* entry (MMT_E_ARG before any HIP
call), and csrc/iounet_dev.h -- the box kernels' arithmetic -- run by a host program under ASan and UBSan."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mmtrack_amd import _lib
from tests.iounet_ref import head_state_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "multi-modal-trakcing-bechmark_amd", "csrc")
D = 0x1000            # a dummy aligned non-null address: a call that got past the checks would report MMT_E_HIP
F = ctypes.c_float


def test_module_imports_without_gpu_and_refuses_cpu_tensors():
    from mmtrack_amd import iounet
    assert iounet.__all__ == ["AtomIoUNet"]
    net = iounet.AtomIoUNet(head_state_dict("real", 1), device="cpu")
    assert (net.c3, net.c4, net.n3, net.n4, net.input_dim) == (256, 256, 256, 256, (32, 32))
    feat = [torch.zeros(1, 256, 12, 12), torch.zeros(1, 256, 6, 6)]
    mod = [torch.ones(1, 256), torch.ones(1, 256)]
    boxes = torch.tensor([[[10.0, 10.0, 30.0, 30.0]]])
    with pytest.raises(NotImplementedError):
        net.predict_iou(mod, feat, boxes)
    with pytest.raises(NotImplementedError):
        net.refine_boxes(mod, feat, boxes)
    with pytest.raises(NotImplementedError):
        net.get_iou_feat([torch.zeros(1, 32, 12, 12), torch.zeros(1, 32, 6, 6)])
    with pytest.raises(NotImplementedError):
        net.get_modulation([torch.zeros(1, 32, 12, 12), torch.zeros(1, 32, 6, 6)], boxes[0])
    small = iounet.AtomIoUNet(head_state_dict("small", 1), device="cpu", precision="fp32")
    assert (small.c3, small.c4, small.n3, small.n4) == (72, 40, 48, 80)
    assert small.convs["conv3_2t"] is None and small.convs["conv3_1t"] is not None   # 72 outputs: no conv kernel


def test_shim_reexports_the_name():
    path = os.path.join(REPO, "multi-modal-trakcing-bechmark_amd", "RGBD", "models", "DeT", "ltr", "models", "bbreg",
                        "__init__.py")
    ns = {}
    exec(compile(open(path).read(), path, "exec"), ns)
    from mmtrack_amd import iounet
    assert ns["AtomIoUNet"] is iounet.AtomIoUNet
    assert sorted(k for k in ns if not k.startswith("__")) == ["AtomIoUNet"]


def test_bad_dimensions_raise_value_error():
    from mmtrack_amd import synth
    from mmtrack_amd.iounet import AtomIoUNet
    for kw in (dict(pred_input_dim=(70, 40)), dict(pred_input_dim=(72, 42)), dict(pred_inter_dim=(40, 80)),
               dict(pred_inter_dim=(48, 72))):
        sd = synth.make_iounet_state_dict(1, input_dim=(32, 32), **dict(dict(pred_input_dim=(72, 40),
                                                                              pred_inter_dim=(48, 80)), **kw))
        with pytest.raises(ValueError):
            AtomIoUNet(sd, device="cpu")
    sd = head_state_dict("small", 1)
    with pytest.raises(ValueError):
        AtomIoUNet(sd, device="cpu", precision="bf16")
    with pytest.raises(ValueError):
        AtomIoUNet(sd, prefix="no_such.", device="cpu")
    sd["bb_regressor.fc3_rt.linear.weight"] = sd["bb_regressor.fc3_rt.linear.weight"][:, :-4].contiguous()
    with pytest.raises(ValueError):
        AtomIoUNet(sd, device="cpu")


def test_ws_bytes_and_the_k_split_without_gpu():
    """mmt_iounet_ws_bytes / mmt_iounet_linear_ws_bytes make no HIP call; the K split a weight shape implies (the
    linear's workspace over rows * N * 4) is the same for 1, 10 and 320 rows, and the predictor's workspace is
    linear in the rows."""
    lib = _lib.load()
    for kd, n in ((6400, 256), (2304, 256), (1800, 48), (360, 80), (1152, 256), (512, 256)):
        splits = {lib.mmt_iounet_linear_ws_bytes(r, kd, n) // (r * n * 4) for r in (1, 10, 320)}
        assert splits == {math.ceil(kd / 128)}, (kd, n, splits)
    one = lib.mmt_iounet_ws_bytes(1, 6400, 2304, 256, 256)
    assert one >= 4 * (2 * (6400 + 2304) + (50 + 18) * 256 + 2 * 256)
    assert lib.mmt_iounet_ws_bytes(10, 6400, 2304, 256, 256) == 10 * one
    assert lib.mmt_iounet_ws_bytes(320, 6400, 2304, 256, 256) == 320 * one
    assert lib.mmt_iounet_ws_bytes(17, 1800, 360, 48, 80) == 17 * lib.mmt_iounet_ws_bytes(1, 1800, 360, 48, 80) > 0
    for bad in ((0, 6400, 2304, 256, 256), (-1, 6400, 2304, 256, 256), (10, 6399, 2304, 256, 256),
                (10, 6400, 2300, 256, 256), (10, 0, 2304, 256, 256), (10, 6400, 2304, 250, 256),
                (10, 6400, 2304, 256, 0), (10, 25 * 6, 2304, 256, 256), (10, 6400, 9 * 2, 256, 256),
                (1 << 20, 6400, 2304, 256, 256)):
        assert lib.mmt_iounet_ws_bytes(*bad) == 0, bad
    for bad in ((0, 6400, 256), (10, 0, 256), (10, 6402, 256), (10, 6400, 0), (10, -4, 256)):
        assert lib.mmt_iounet_linear_ws_bytes(*bad) == 0, bad


def _linear(lib, **over):
    a = dict(X=D, rows=10, Kd=1800, W=D, N=48, bias=D, scale=D, rpg=10, bins=25, relu=1, Y=D, ws=D,
             ws_bytes=15 * 10 * 48 * 4)
    a.update(over)
    return lib.mmt_iounet_linear(a["X"], a["rows"], a["Kd"], a["W"], a["N"], a["bias"], a["scale"], a["rpg"], a["bins"],
                                 a["relu"], a["Y"], a["ws"], a["ws_bytes"], None)


def _head(**over):
    h = _lib.MmtIounetHead(D, D, D, D, D, 0.5, 72, 40, 48, 80)
    for k, v in over.items():
        setattr(h, k, v)
    return h


def _feat(B=2, **over):
    l3 = _lib.MmtIounetMap(D, 12, 12, 72, 12 * 72, 144 * 72)
    l4 = _lib.MmtIounetMap(D, 6, 6, 40, 6 * 40, 36 * 40)
    for k, v in over.items():
        lvl, field = k.split("_")
        setattr(l3 if lvl == "l3" else l4, field, v)
    return _lib.MmtIounetFeat(B, 0, l3, l4)


def _calls(lib, head=None, feat=None, null_head=False, null_feat=False, **over):
    """(predict's, refine's) return codes for one set of arguments."""
    h, f = head or _head(), feat or _feat()
    a = dict(mod3=D, mod4=D, boxes=D, P=10, grad_iou=D, iou=D, grad_boxes=D, ws=D, iters=5, sp=1.0, ss=1.0, decay=1.0,
             out=D)
    a.update(over)
    need = lib.mmt_iounet_ws_bytes(max(f.B, 1) * max(a["P"], 1), 1800, 360, 48, 80)
    wsb = a.get("ws_bytes", need)
    hp = None if null_head else ctypes.byref(h)
    fp = None if null_feat else ctypes.byref(f)
    p = lib.mmt_iounet_predict(hp, fp, a["mod3"], a["mod4"], a["boxes"], a["P"], a["grad_iou"], a["iou"],
                               a["grad_boxes"], a["ws"], wsb, None)
    r = lib.mmt_iounet_refine(hp, fp, a["mod3"], a["mod4"], a["boxes"], a["P"], a["iters"], F(a["sp"]), F(a["ss"]),
                              F(a["decay"]), a["out"], a["iou"], a["ws"], wsb, None)
    return p, r


def test_entries_reject_bad_arguments_without_gpu():
    """Every mmt_iounet_* entry checks its arguments before any HIP call: each rejected call below returns MMT_E_ARG
    over dummy pointers on a machine without a GPU (a call that got past the checks would report MMT_E_HIP or die)."""
    lib, E = _lib.load(), _lib.MMT_E_ARG
    for over in (dict(X=None), dict(W=None), dict(Y=None), dict(ws=None), dict(rows=0), dict(rows=-3), dict(Kd=0),
                 dict(Kd=1802), dict(N=0), dict(X=D + 4), dict(W=D + 8), dict(ws=D + 4), dict(ws_bytes=15 * 10 * 48 * 4 - 1),
                 dict(ws_bytes=0), dict(rpg=0), dict(bins=0), dict(bins=7), dict(rows=1 << 20)):
        assert _linear(lib, **over) == E, over
    both = [dict(mod3=None), dict(mod4=None), dict(boxes=None), dict(iou=None), dict(ws=None), dict(P=0), dict(P=-1),
            dict(boxes=D + 4), dict(ws=D + 8), dict(ws_bytes=0), dict(ws_bytes=1000), dict(null_head=True),
            dict(null_feat=True), dict(feat=_feat(B=0)), dict(feat=_feat(B=-2)), dict(feat=_feat(B=1 << 18)),
            dict(feat=_feat(l3_p=None)), dict(feat=_feat(l4_p=None)), dict(feat=_feat(l3_p=D + 4)),
            dict(feat=_feat(l3_H=0)), dict(feat=_feat(l4_W=0)), dict(feat=_feat(l3_pix=68)), dict(feat=_feat(l3_pix=74)),
            dict(feat=_feat(l3_row=11 * 72)), dict(feat=_feat(l4_img=35 * 40)), dict(feat=_feat(l4_row=6 * 40 + 2)),
            dict(head=_head(w3=None)), dict(head=_head(b3=None)), dict(head=_head(w4=None)), dict(head=_head(b4=None)),
            dict(head=_head(wp=None)), dict(head=_head(w3=D + 4)), dict(head=_head(w4=D + 4)), dict(head=_head(c3=0)),
            dict(head=_head(c3=70)), dict(head=_head(c4=-4)), dict(head=_head(n3=0)), dict(head=_head(n3=40)),
            dict(head=_head(n4=72)), dict(head=_head(bp=math.nan)), dict(head=_head(bp=math.inf))]
    for over in both:
        assert _calls(lib, **over) == (E, E), over
    assert _calls(lib, grad_boxes=D + 4)[0] == E
    for over in (dict(out=None), dict(out=D + 4), dict(iters=0), dict(iters=-1), dict(iters=1025), dict(sp=math.nan),
                 dict(ss=math.inf), dict(decay=math.nan)):
        assert _calls(lib, **over)[1] == E, over


def _fmt(v):
    v = float(v)
    return "nan" if math.isnan(v) else ("inf" if v == math.inf else ("-inf" if v == -math.inf else repr(v)))


def test_box_arithmetic_on_the_host_under_sanitizers(tmp_path):
    """tests/iounet_host_check.cpp calls the functions of iounet_dev.h that the box kernels call, on ordinary boxes and
    on boxes with NaN, infinite, huge and negative values: a clean exit under ASan + UBSan, and the bits of the same
    float32 operations done one at a time in numpy (the order the reference's torch operations round in)."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        cxx = "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "iounet_host_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(REPO, "tests", "iounet_host_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.uniform(1, 200, (12, 4)), rng.normal(0, 3, (12, 8))], axis=1).astype(np.float32)
    odd = np.array([[math.nan, 5, 10, 10], [5, 5, math.inf, 10], [5, 5, -10, 10], [1e30, 1e30, 3e38, 3e38],
                    [-500, -500, 10, 10], [5, -math.inf, 10, math.nan]], dtype=np.float32)
    rows = np.concatenate([rows, np.concatenate([odd, rng.normal(0, 3, (6, 8)).astype(np.float32)], axis=1)])
    P, sp, ss = 5, np.float32(0.7), np.float32(0.3)
    text = "".join(" ".join(_fmt(v) for v in r) + "\n" for r in rows)
    run = subprocess.run([exe, str(P), repr(float(sp)), repr(float(ss))], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == 3 * len(rows) + 1 and lines[-1] == "ksplit 1 1 2 3 18 50"
    got = {k: np.array([[np.float32(v) for v in ln.split()[1:]] for ln in lines[:-1] if ln.startswith(k)], np.float32)
           for k in ("roi", "grad", "step")}
    with np.errstate(all="ignore"):
        box, g3, g4 = rows[:, :4], rows[:, 4:8], rows[:, 8:]
        roi = np.stack([(np.arange(len(rows)) // P).astype(np.float32), box[:, 0], box[:, 1], box[:, 0] + box[:, 2],
                        box[:, 1] + box[:, 3]], axis=1)
        grad = np.stack([(g3[:, 0] + g3[:, 2]) + (g4[:, 0] + g4[:, 2]), (g3[:, 1] + g3[:, 3]) + (g4[:, 1] + g4[:, 3]),
                         g3[:, 2] + g4[:, 2], g3[:, 3] + g4[:, 3]], axis=1)
        step = np.array([sp, sp, ss, ss], np.float32)
        out = box + (step * grad) * box[:, [2, 3, 2, 3]]
    for k, want in (("roi", roi), ("grad", grad), ("step", out)):
        assert want.dtype == np.float32 and np.array_equal(got[k], want, equal_nan=True), k
