"""Operator-level tests of the frame-side kernels (csrc/imaging.hip): crop_kernel<false / true>, geometry_kernel and
decode_kernel, through mmt_op_crop_patchify / mmt_op_crop_geometry / mmt_op_decode (GPU), and the host's
mmt_crop_geometry_host (no GPU: the one unmarked test).

Every output buffer starts as a sentinel (NaN, 0xFFFF, the byte 0xA5, -7 for index arrays) and is one row / record
longer than the launch needs; every test checks that what it does not own still holds the sentinel and that what it
owns equals the reference (which never holds a 16-bit or fp32 sentinel).

Crop: everything is bitwise.  The reference is oracle.crop.sample_target (its padding and its cv2 restatement; at
output sizes the engine never uses, that formula is the specification), oracle.crop.preprocess and
torch.nn.functional.unfold(., 16, stride=16) as an independent statement of the patch layout; the f16x3 halves are the
host split of t * 4096, the bf16 tokens t.bfloat16().  A crop given as x1, y1, crop_sz is the oracle's crop of the box
(x1, y1, crop_sz, crop_sz) at factor 1 (asserted).  The geometry cases of the issue run on a 541 x 577 frame (the
smallest on which a 512-pixel crop is interior); the other frames are 97 x 131 and 60 x 45.

Geometry: integers equal, rf equal as double bits, between oracle.crop.crop_geometry (python round), the host function
(nearbyint) and geometry_of on the device (rint), on a list holding the four half-way cases that tell half-to-even
from truncation, floor(v + 0.5) and half-away.

Decode values against float64 on the same fp32 inputs.  Bar of a conv5 sum: (32 + 2) 2^-24 (sum |h_k w_k| + |b|);
offset maps: that bar; sigmoid maps: a quarter of it + 4 * 2^-24.  The argmax reference is the float64 argmax of
hann * ctr; each case's top-two margin is asserted (on the reference alone) to exceed twice the response bar
hann (bar_ctr / 4 + 4 * 2^-24) + 2^-24 resp.  The state update is compared as double bits with oracle/tracker.py's
arithmetic ((tensor(res[:4]) * search_size / rf).tolist(), map_box_back, clip_box with margin 10).

Measured on the MI355X (fs in 3, 16, 17, 24; B in 1, 3; seeds 100 fs + B): worst |error| / bar over all cases: ctr map
0.044, size maps 0.066, offset maps 0.091.  Argmax margins as multiples of twice the response bar, per case in that
order: 3830, 8392, 34812, 2376, 19903, 343, 447, 206 (the smallest of a case's sequences).  Every bitwise crop,
geometry, gather and state comparison held as written: no kernel change was needed.

Each of these memory-safe arithmetic changes to imaging.hip, built one at a time into a scratch library, was seen to
fail the tests named (and no others):
  * H - 2 -> H - 1 in crop_px: test_crop_geometries, test_crop_sizes_frames_strides (all but 32),
    test_crop_fused_equals_geometry_then_crop;
  * the channel plane (c % 3) * 256 -> ((c + 1) % 3) * 256: the same three, every case;
  * rint -> round in geometry_of: test_crop_geometry_device_matches_oracle, test_crop_geometry_sequence_counts
    [256, 257], test_crop_geometry_ring, test_crop_fused_equals_geometry_then_crop;
  * resp > best -> >=: test_decode_argmax_ties[17-ones], [24-ones] (the set {5, 261} of one thread's strided loop);
  * ties to the higher index in the LDS reduction: test_decode_argmax_ties (all eight), test_decode_clamp_ends;
  * br_of {0, 1, 1, 2, 2} -> {0, 1, 2, 1, 2}: test_decode_values_and_argmax (all eight);
  * the margins of the two x clamps of update_state swapped: test_decode_state_update (both);
  * the fused crop skipping the rf store: test_crop_fused_equals_geometry_then_crop (all four).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import crop as ocrop
from oracle import tracker as otracker
from oracle import vipt as ov
from test_gpu_tokens import split_host

gpu = pytest.mark.gpu

U = 2.0 ** -24
FILL8 = 0xA5
E_ARG, E_BOX = -1, -5


@pytest.fixture(scope="module")
def lib():
    from mmtrack_amd import _lib
    return _lib.load()


def L():
    from mmtrack_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ device records
def to_dev(records, cls, extra=1):
    """The records as device bytes, followed by `extra` sentinel records."""
    raw = b"".join(bytes(r) for r in records) + bytes([FILL8]) * (ctypes.sizeof(cls) * extra)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def from_dev(t, cls, n):
    raw, sz = t.cpu().numpy().tobytes(), ctypes.sizeof(cls)
    return [cls.from_buffer_copy(raw[i * sz:(i + 1) * sz]) for i in range(n)]


def guard_ok(t, cls, n, what):
    assert (t[n * ctypes.sizeof(cls):] == FILL8).all(), f"{what}: a store past the last record"


def sentinel(cls, n):
    return to_dev([], cls, n)


def ints(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def bits16(rows):
    """rows + 1 rows of 768 16-bit words, all 0xFFFF."""
    return torch.full((rows + 1, 768), -1, dtype=torch.int16, device="cuda")


def dbits(x):
    return np.float64(x).view(np.int64).item()


# ------------------------------------------------------------------------------------------ frames
FRAME_SHAPES = {"big": (541, 577, 6, 1), "a": (97, 131, 6, 2), "b": (60, 45, 6, 3), "c": (75, 88, 6, 4),
                "big3": (541, 577, 3, 5), "a3": (97, 131, 3, 6), "b3": (60, 45, 3, 7), "c3": (75, 88, 3, 8)}


@functools.lru_cache(maxsize=None)
def frame(key):
    H, W, C, seed = FRAME_SHAPES[key]
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(H, W, C), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def frame_dev(key, pad):
    """The frame on the device with a row stride of W * C + pad bytes (the gap holds a byte no test expects)."""
    im = frame(key)
    H, W, C = im.shape
    buf = np.full((H, W * C + pad), 0x3C, np.uint8)
    buf[:, :W * C] = im.reshape(H, W * C)
    return torch.from_numpy(buf).cuda()


def crop_param(key, pad, x1=-99, y1=-99, cs=-99):
    H, W, C = frame(key).shape
    return L().MmtCropParam(frame_dev(key, pad).data_ptr(), W * C + pad, H, W, C, x1, y1, cs, 0)


def tokens_of(patch):
    """The fp32 token rows of a uint8 crop: [(O / 16)^2][768] per 3-channel half, by preprocess + unfold."""
    t = ocrop.preprocess(patch)
    return [F.unfold(t[:, 3 * k:3 * k + 3], 16, stride=16)[0].T.contiguous() for k in range(patch.shape[2] // 3)]


@functools.lru_cache(maxsize=None)
def crop_expected(key, x1, y1, cs, O):
    """(uint8 crop, token rows) of the oracle for the crop x1, y1, crop_sz of a frame."""
    im = frame(key)
    H, W = im.shape[:2]
    assert y1 <= H - 2 and y1 + cs >= 1 and x1 <= W - 2 and x1 + cs >= 1, "the crop misses the frame: out of contract"
    box = [float(x1), float(y1), float(cs), float(cs)]
    assert ocrop.crop_geometry(box, 1.0, O)[:3] == (x1, y1, cs)
    patch, _ = ocrop.sample_target(im, box, 1.0, O)
    assert patch.shape == (O, O, im.shape[2])
    return patch, tokens_of(patch)


def crop_buffers(B, O, C, mode, rps):
    bufs = dict(A_rgb=bits16(B * rps), A_aux=bits16(B * rps), A_rgb_lo=None, A_aux_lo=None,
                dbg=torch.full((B * O * O * C + O * C,), FILL8, dtype=torch.uint8, device="cuda"))
    if mode == "f16x3":
        bufs["A_rgb_lo"], bufs["A_aux_lo"] = bits16(B * rps), bits16(B * rps)
    return bufs


def call_crop(lib, params_t, bufs, B, O, C, rps, row0, geom=None, expect=0, dbg=True):
    a = L().MmtCropArgs(P(params_t), B, O, C, P(bufs["A_rgb"]), P(bufs["A_aux"]), P(bufs["A_rgb_lo"]),
                        P(bufs["A_aux_lo"]), rps, row0, P(bufs["dbg"]) if dbg else None)
    rc = lib.mmt_op_crop_patchify(ctypes.byref(a), ctypes.byref(geom) if geom is not None else None, _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc


def untouched(bufs):
    return all((v == (FILL8 if k == "dbg" else -1)).all().item() for k, v in bufs.items() if v is not None)


def check_crop(bufs, expected, O, C, mode, rps, row0):
    """expected: per sequence (uint8 crop, token rows).  Owned rows equal the reference, everything else untouched."""
    B, npatch = len(expected), (O // 16) ** 2
    dbg = bufs["dbg"].cpu().numpy()
    assert (dbg[B * O * O * C:] == FILL8).all(), "dbg_patch: a store past the last crop"
    own = torch.zeros(B * rps + 1, dtype=torch.bool)
    for b in range(B):
        own[b * rps + row0:b * rps + row0 + npatch] = True
    names = ["A_rgb", "A_aux"]
    for k, name in enumerate(names):
        for suffix in ("", "_lo"):
            buf = bufs[name + suffix]
            if buf is None:
                continue
            got = buf.cpu()
            if k >= C // 3:   # the aux buffers of a 3-channel launch
                assert (got == -1).all(), f"{name}{suffix}: written by a 3-channel launch"
                continue
            assert (got[~own] == -1).all(), f"{name}{suffix}: a row outside row0 .. row0 + patches was written"
            for b in range(B):
                t = expected[b][1][k]
                if mode == "f16x3":
                    want = split_host(t, 4096.0)[0 if suffix == "" else 1].view(torch.int16)
                else:
                    want = t.bfloat16().view(torch.int16)
                rows = got[b * rps + row0:b * rps + row0 + npatch]
                assert torch.equal(rows, want), f"{name}{suffix} sequence {b}: {(rows != want).sum().item()} words differ"
    for b in range(B):
        got = dbg[b * O * O * C:(b + 1) * O * O * C].reshape(O, O, C)
        np.testing.assert_array_equal(got, expected[b][0], err_msg=f"dbg_patch sequence {b}")


def geometry_cases(H, W, O):
    """The issue's crop geometries (x1, y1, crop_sz) for an H x W frame and output size O."""
    cs_dn, cs_e = int(O * 1.37) + 1, O + 13
    g = [(40, 33, cs_dn),                                   # interior, non-integer down-scale
         (20, 11, 2 * O),                                   # exact 2x (INTER_AREA), interior
         (-37, 15, 2 * O), (25, -21, 2 * O), (W + 50 - 2 * O, 9, 2 * O), (13, H + 33 - 2 * O, 2 * O),   # ... each edge
         (7, 9, O),                                         # crop_sz == out_sz
         (50, 60, O // 3 + 1),                              # up-scale
         (50, 60, 1), (51, 61, 2),
         (W - 1 - cs_e, 5, cs_e), (W - cs_e, 5, cs_e), (W + 1 - cs_e, 5, cs_e),     # x2 = W - 1, W, W + 1
         (6, H - 1 - cs_e, cs_e), (6, H - cs_e, cs_e), (6, H + 1 - cs_e, cs_e),     # y2 likewise
         (-9, -14, cs_e),                                   # x1 < 0 and y1 < 0
         (-60, -70, max(H, W) + 123)]                       # larger than the frame on all sides
    for x1, y1, cs in g[1:6]:
        assert cs == 2 * O
    assert g[1][0] > 0 and g[1][1] > 0 and g[1][0] + 2 * O < W - 1 and g[1][1] + 2 * O < H - 1
    assert g[4][0] + 2 * O > W and g[5][1] + 2 * O > H
    return g


# ------------------------------------------------------------------------------------------ crop, not fused
@gpu
@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
@pytest.mark.parametrize("O", [48, 256])
def test_crop_geometries(lib, O, mode):
    """Every crop geometry of the list in one launch (one sequence each) at the search placement row0 = Lz inside a
    longer rows_per_seq: the uint8 crop, the token values / halves and the patch layout, bitwise."""
    H, W, C = frame("big").shape
    geos = geometry_cases(H, W, O)
    B, npatch = len(geos), (O // 16) ** 2
    row0 = npatch // 4 if npatch >= 4 else 4
    rps = row0 + npatch + 3
    params = to_dev([crop_param("big", 0, *g) for g in geos], L().MmtCropParam)
    bufs = crop_buffers(B, O, C, mode, rps)
    call_crop(lib, params, bufs, B, O, C, rps, row0)
    check_crop(bufs, [crop_expected("big", *g, O) for g in geos], O, C, mode, rps, row0)


SIZE_CASES = [  # O, C, template placement (row0 = 0, rows_per_seq = patches)?
    (32, 6, True), (48, 6, False), (128, 6, True), (256, 6, False), (192, 3, True), (384, 3, False)]


@gpu
@pytest.mark.parametrize("mode", ["f16x3", "bf16"])
@pytest.mark.parametrize("O,C,template", SIZE_CASES)
def test_crop_sizes_frames_strides(lib, O, C, template, mode):
    """B = 3 with three frames (97 x 131, 60 x 45, 75 x 88), three row strides (tight, W * C + 5, W * C + 64) and three
    geometries in one launch; the engine's output sizes and 32 / 48; both channel counts (the aux buffers of a
    3-channel launch stay untouched); template (row0 = 0) and search (row0 = Lz) placement."""
    s = "3" if C == 3 else ""
    seqs = [("a" + s, 5, -11, 20, O + 7),            # overhangs the left edge, stride W * C + 5
            ("b" + s, 0, -30, -25, 2 * O),           # larger than the 60 x 45 frame on all sides for O >= 48, exact 2x
            ("c" + s, 64, 10, 12, O // 2 + 3)]       # interior up-scale where the frame holds it
    npatch = (O // 16) ** 2
    row0, rps = (0, npatch) if template else (npatch // 4 + 1, npatch // 4 + 1 + npatch + 2)
    params = to_dev([crop_param(k, pad, x1, y1, cs) for k, pad, x1, y1, cs in seqs], L().MmtCropParam)
    bufs = crop_buffers(3, O, C, mode, rps)
    call_crop(lib, params, bufs, 3, O, C, rps, row0)
    check_crop(bufs, [crop_expected(k, x1, y1, cs, O) for k, pad, x1, y1, cs in seqs], O, C, mode, rps, row0)


@gpu
def test_crop_rejects(lib):
    """Each bad argument is MMT_E_ARG and nothing is launched: every buffer keeps its sentinel."""
    O, C, rps = 32, 6, 6
    good = to_dev([crop_param("a", 0, 3, 4, 40)], L().MmtCropParam)
    bufs = crop_buffers(1, O, C, "f16x3", rps)

    def bad(params=good, B=1, O=O, C=C, rps=rps, row0=1, drop=(), geom=None):
        b = {k: (None if k in drop else v) for k, v in bufs.items()}
        call_crop(lib, params, b, B, O, C, rps, row0, geom=geom, expect=E_ARG)
        assert untouched(bufs)

    for o in (0, -16, 24, 40):
        bad(O=o)
    for c in (0, 1, 4, 5, 7):
        bad(C=c)
    bad(drop=("A_aux", "A_aux_lo"))           # C == 6 without an aux buffer
    bad(drop=("A_aux_lo",))                   # halves for one buffer only
    bad(drop=("A_rgb",))
    bad(row0=3)                               # row0 + 4 patches > rows_per_seq
    bad(row0=-1)
    bad(B=0)
    bad(params=None)
    bad(params=to_dev([crop_param("a3", 0, 3, 4, 40)], L().MmtCropParam))     # a 3-channel frame in a 6-channel launch
    bad(params=to_dev([crop_param("a", 0, 3, 4, 0)], L().MmtCropParam))       # crop_sz < 1
    p = crop_param("a", 0, 3, 4, 40)
    p.stride = p.W * p.C - 1
    bad(params=to_dev([p], L().MmtCropParam))
    p = crop_param("a", 0, 3, 4, 40)
    p.frame = None
    bad(params=to_dev([p], L().MmtCropParam))
    # fused: no state; a ring counter outside [0, kring); a ring pitch below B
    st = to_dev([L().MmtSeqState((ctypes.c_double * 4)(10, 10, 20, 20), 0.0, 0, 0)], L().MmtSeqState)
    bad(geom=L().MmtGeomArgs(None, 4.0, L().MmtRingArgs(), 0, None, None, 0, 0))
    bad(geom=L().MmtGeomArgs(P(st), 0.0, L().MmtRingArgs(), 0, None, None, 0, 0))
    ctr, cur = ints([3]), ints([0])
    ring = L().MmtRingArgs(P(good), None, P(ctr), P(cur), 3, 1)
    bad(geom=L().MmtGeomArgs(P(st), 4.0, ring, 1, None, None, 0, 0))
    ctr = ints([0])
    ring = L().MmtRingArgs(P(good), None, P(ctr), P(cur), 3, 0)
    bad(geom=L().MmtGeomArgs(P(st), 4.0, ring, 1, None, None, 0, 0))
    gi = ints([-7] * 5)
    bad(geom=L().MmtGeomArgs(P(st), 4.0, L().MmtRingArgs(), 0, P(gi), None, 1, 4))   # gidx without slot2pos
    assert (gi == -7).all()
    assert lib.mmt_op_crop_patchify(None, None, _stream()) == E_ARG


# ------------------------------------------------------------------------------------------ geometry
# (box, factor, out_sz, expected error)
GEO_LIST = [
    ((11.0, 20.0, 25.0, 25.0), 4.0, 256, 0),      # v = -26.5 -> -26
    ((10.0, 20.0, 25.0, 25.0), 4.0, 256, 0),      # v = -27.5 -> -28
    ((64.0, 65.0, 25.0, 25.0), 4.0, 256, 0),      # v = 26.5 -> 26 (x), 27.5 -> 28 (y)
    ((63.0, 65.0, 25.0, 25.0), 4.0, 256, 0),      # v = 25.5 -> 26
    ((100.0, 90.0, 32.0, 32.0), 4.0, 256, 0),     # sqrt * factor exactly 128: ceil keeps it
    ((100.0, 90.0, 32.0 * (1 + 2.0 ** -50), 32.0), 4.0, 256, 0),   # just above an integer: 129
    ((300.25, 200.75, 41.3, 29.9), 4.0, 256, 0),
    ((-40.5, -12.25, 60.0, 17.0), 4.0, 256, 0),
    ((5.0, 6.0, 0.01, 0.01), 4.0, 256, 0),        # crop_sz 1
    ((5.0, 6.0, 0.0, 7.0), 4.0, 256, E_BOX),      # w = 0
    ((5.0, 6.0, -3.0, 7.0), 4.0, 256, E_BOX),     # w h < 0: NaN
    ((5.0, 6.0, 3e5, 3e5), 4.0, 256, E_ARG),      # crop_sz 1.2e6
    ((11.0, 20.0, 25.0, 25.0), 2.0, 128, 0),      # factor 2: cs 50, v = -1.5 -> -2, 7.5 -> 8
    ((12.0, 21.0, 25.0, 25.0), 2.0, 128, 0),      # v = -0.5 -> 0 (x), 8.5 -> 8 (y)
    ((100.0, 90.0, 64.0, 64.0), 2.0, 128, 0),     # exactly 128
    ((33.3, 44.4, 17.7, 91.1), 2.0, 128, 0),
    ((5.0, 6.0, 0.0, 0.0), 2.0, 128, E_BOX),
]
TIES = {0: (-26, None), 1: (-28, None), 2: (26, 28), 3: (26, 28)}


def geometry_expected(box, factor, out_sz, err):
    """(x1, y1, crop_sz, rf) of oracle.crop.crop_geometry; for the error boxes, the harmless crop the engine forms
    (the oracle raises, as the reference does)."""
    if err:
        w, h = box[2], box[3]
        assert w * h < 0 or math.ceil(math.sqrt(w * h) * factor) < 1 or math.ceil(math.sqrt(w * h) * factor) > 1e6
        if err == E_BOX:
            with pytest.raises(Exception):
                ocrop.crop_geometry(box, factor, out_sz)
        return 0, 0, 1, 1.0
    return ocrop.crop_geometry(box, factor, out_sz)


def test_crop_geometry_host_matches_oracle(lib):
    """No GPU: mmt_crop_geometry_host (what the engine's host path calls) == oracle.crop.crop_geometry: integers
    equal, rf as double bits, the error codes; the four half-way boxes round half to even."""
    for i, (box, factor, out_sz, err) in enumerate(GEO_LIST):
        x1, y1, cs, rf = ctypes.c_int(-99), ctypes.c_int(-99), ctypes.c_int(-99), ctypes.c_double(-99.0)
        rc = lib.mmt_crop_geometry_host((ctypes.c_double * 4)(*box), factor, out_sz, ctypes.byref(x1), ctypes.byref(y1),
                                        ctypes.byref(cs), ctypes.byref(rf))
        assert rc == err, (box, rc)
        ex1, ey1, ecs, erf = geometry_expected(box, factor, out_sz, err)
        assert (x1.value, y1.value, cs.value) == (ex1, ey1, ecs), box
        assert dbits(rf.value) == dbits(erf), box
        if i in TIES:
            assert x1.value == TIES[i][0] and TIES[i][1] in (None, y1.value)
    assert lib.mmt_crop_geometry_host(None, 4.0, 256, None, None, None, None) == E_ARG


def seq_state(box, rf=float("nan"), err=77):
    return L().MmtSeqState((ctypes.c_double * 4)(*box), rf, err, 0)


def run_geometry(lib, boxes, factor, out_sz, ring=None, Lz=0, Lx=0, params=None, expect=0):
    """geometry_kernel over the boxes; returns (params records, state records, gidx, slot2pos) read back."""
    n = len(boxes)
    params_t = to_dev(params or [crop_param("a", 0) for _ in boxes], L().MmtCropParam)
    state_t = to_dev([seq_state(b) for b in boxes], L().MmtSeqState)
    gidx = ints([-7] * (n * Lx + 1)) if Lx else None
    s2p = ints([-7] * (n * Lx + 1)) if Lx else None
    rc = lib.mmt_op_crop_geometry(P(params_t), P(state_t), n, factor, out_sz, ctypes.byref(ring) if ring else None,
                                  P(gidx), P(s2p), Lz, Lx, _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    guard_ok(params_t, L().MmtCropParam, n, "params")
    guard_ok(state_t, L().MmtSeqState, n, "state")
    return params_t, state_t, gidx, s2p


def check_geometry(params_t, state_t, cases):
    n = len(cases)
    for (box, factor, out_sz, err), p, s in zip(cases, from_dev(params_t, L().MmtCropParam, n),
                                                from_dev(state_t, L().MmtSeqState, n)):
        ex1, ey1, ecs, erf = geometry_expected(box, factor, out_sz, err)
        assert (p.x1, p.y1, p.crop_sz) == (ex1, ey1, ecs), box
        assert dbits(s.rf) == dbits(erf) and s.err == err, box
        assert [dbits(v) for v in s.box] == [dbits(v) for v in box], "the state's box is not the kernel's to change"


@gpu
@pytest.mark.parametrize("factor,out_sz", [(4.0, 256), (2.0, 128)])
def test_crop_geometry_device_matches_oracle(lib, factor, out_sz):
    """geometry_kernel on the list of the host test: the same integers, rf bits and error codes; the frame fields
    of params are left alone without a ring."""
    cases = [c for c in GEO_LIST if c[1] == factor]
    params_t, state_t, _, _ = run_geometry(lib, [c[0] for c in cases], factor, out_sz)
    check_geometry(params_t, state_t, cases)
    want = crop_param("a", 0)
    for p in from_dev(params_t, L().MmtCropParam, len(cases)):
        assert (p.frame, p.stride, p.H, p.W, p.C) == (want.frame, want.stride, want.H, want.W, want.C)


@gpu
@pytest.mark.parametrize("n", [1, 256, 257])
def test_crop_geometry_sequence_counts(lib, n):
    """The 256-thread loops: n sequences (one, exactly one pass, one sequence into the second pass) and n * Lx index
    words with Lz = 4, Lx = 9."""
    Lz, Lx = 4, 9
    rng = np.random.Generator(np.random.PCG64(n))
    cases = [((float(rng.integers(0, 600)) + 0.5 * (i % 2), float(rng.integers(0, 400)), float(rng.integers(8, 90)),
               float(rng.integers(8, 90))), 4.0, 256, 0) for i in range(n)]
    params_t, state_t, gidx, s2p = run_geometry(lib, [c[0] for c in cases], 4.0, 256, Lz=Lz, Lx=Lx)
    check_geometry(params_t, state_t, cases)
    j = torch.arange(Lx, dtype=torch.int32).repeat(n)
    assert torch.equal(gidx[:-1].cpu(), j) and torch.equal(s2p[:-1].cpu(), j + Lz)
    assert gidx[-1].item() == -7 and s2p[-1].item() == -7


def ring_of(entries, kring, pitch, ctr0):
    """A ring in ordinary device memory: entries[e] = the descriptors of ring entry e (pitch each)."""
    assert len(entries) == kring and all(len(e) == pitch for e in entries)
    rp = to_dev([p for e in entries for p in e], L().MmtCropParam)
    ctr, cur = ints([ctr0]), ints([-7])
    return L().MmtRingArgs(P(rp), None, P(ctr), P(cur), kring, pitch), (rp, ctr, cur)


RING_FRAMES = [("a", 0), ("b", 5), ("c", 64), ("big", 0)]


def ring_entries(kring=3, pitch=4):
    return [[crop_param(*RING_FRAMES[(e + i) % 4], x1=1000 + e, y1=2000 + i, cs=3000) for i in range(pitch)]
            for e in range(kring)]


@gpu
def test_crop_geometry_ring(lib):
    """Three launches over a ring of kring = 3, pitch = 4 (device memory standing in for the pinned ring): each copies
    the frame fields of entry ctr into params, leaves x1 / y1 / crop_sz to the geometry, sets *cur and advances ctr
    0 -> 1 -> 2 -> 0."""
    entries = ring_entries()
    ring, (rp, ctr, cur) = ring_of(entries, 3, 4, 0)
    cases = [c for c in GEO_LIST if c[1] == 4.0][:3]
    params_t = to_dev([L().MmtCropParam() for _ in cases], L().MmtCropParam)
    for launch in range(3):
        state_t = to_dev([seq_state(c[0]) for c in cases], L().MmtSeqState)
        rc = lib.mmt_op_crop_geometry(P(params_t), P(state_t), 3, 4.0, 256, ctypes.byref(ring), None, None, 0, 0,
                                      _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert cur.item() == launch and ctr.item() == (launch + 1) % 3
        check_geometry(params_t, state_t, cases)
        for i, p in enumerate(from_dev(params_t, L().MmtCropParam, 3)):
            w = entries[launch][i]
            assert (p.frame, p.stride, p.H, p.W, p.C) == (w.frame, w.stride, w.H, w.W, w.C), (launch, i)
        guard_ok(params_t, L().MmtCropParam, 3, "params")
    assert bytes(rp.cpu().numpy()[:12 * 48]) == b"".join(bytes(p) for e in entries for p in e), "the ring is read only"


@gpu
def test_crop_geometry_rejects(lib):
    boxes = [(10.0, 10.0, 20.0, 20.0)]
    pt, st = to_dev([crop_param("a", 0)], L().MmtCropParam), to_dev([seq_state(boxes[0])], L().MmtSeqState)
    before = (pt.clone(), st.clone())
    gi, sp = ints([-7] * 10), ints([-7] * 10)
    ring, (rp, ctr, cur) = ring_of(ring_entries(), 3, 4, 3)          # counter out of range
    small, _keep = ring_of(ring_entries(3, 1), 3, 1, 0)              # pitch below n = 2
    calls = [(None, P(st), 1, 4.0, 256, None, None, None, 0, 0), (P(pt), None, 1, 4.0, 256, None, None, None, 0, 0),
             (P(pt), P(st), 0, 4.0, 256, None, None, None, 0, 0), (P(pt), P(st), 1, 0.0, 256, None, None, None, 0, 0),
             (P(pt), P(st), 1, 4.0, 0, None, None, None, 0, 0), (P(pt), P(st), 1, 4.0, 256, None, P(gi), None, 4, 9),
             (P(pt), P(st), 1, 4.0, 256, None, P(gi), P(sp), 4, 0), (P(pt), P(st), 1, 4.0, 256, None, P(gi), P(sp), -1, 9),
             (P(pt), P(st), 1, 4.0, 256, ctypes.byref(ring), None, None, 0, 0),
             (P(pt), P(st), 2, 4.0, 256, ctypes.byref(small), None, None, 0, 0)]
    for c in calls:
        assert lib.mmt_op_crop_geometry(*c, _stream()) == E_ARG, c
    torch.cuda.synchronize()
    assert torch.equal(pt, before[0]) and torch.equal(st, before[1])
    assert (gi == -7).all() and (sp == -7).all() and ctr.item() == 3 and cur.item() == -7


# ------------------------------------------------------------------------------------------ fused == separate
FUSED_BOXES = [(200.25, 150.5, 41.0, 29.0), (5.0, 6.0, 0.0, 7.0), (500.0, 480.0, 70.0, 33.0)]   # the second: MMT_E_BOX


@gpu
@pytest.mark.parametrize("use_ring", [0, 1])
@pytest.mark.parametrize("factor,O,mode", [(4.0, 256, "f16x3"), (2.0, 128, "bf16")])
def test_crop_fused_equals_geometry_then_crop(lib, factor, O, mode, use_ring):
    """crop_kernel<true> against geometry_kernel + crop_kernel<false> on three sequences (one a too-small box, which
    leaves the other two alone): tokens and the uint8 crop bitwise, params / state records byte for byte, gidx /
    slot2pos equal.  With the ring: the frame fields come from entry ctr, *cur is set and ctr is left for decode."""
    C, B, npatch = 6, 3, (O // 16) ** 2
    Lz, Lx = npatch // 4, npatch
    row0, rps = Lz, Lz + npatch + 1
    entries = ring_entries()
    entries[1][:3] = [crop_param("big", 0, x1=-5, y1=-6, cs=-7), crop_param("big", 5, x1=-5, y1=-6, cs=-7),
                      crop_param("big", 0, x1=-5, y1=-6, cs=-7)]
    host = [crop_param("big", 0), crop_param("big", 5), crop_param("big", 0)]
    blank = [L().MmtCropParam() for _ in range(B)]

    def fresh():
        return (to_dev(blank if use_ring else host, L().MmtCropParam),
                to_dev([seq_state(b) for b in FUSED_BOXES], L().MmtSeqState), ints([-7] * (B * Lx + 1)),
                ints([-7] * (B * Lx + 1)))

    # separate
    p_s, s_s, g_s, t_s = fresh()
    ring_s, keep_s = ring_of(entries, 3, 4, 1)
    rc = lib.mmt_op_crop_geometry(P(p_s), P(s_s), B, factor, O, ctypes.byref(ring_s) if use_ring else None, P(g_s),
                                  P(t_s), Lz, Lx, _stream())
    assert rc == 0
    bufs_s = crop_buffers(B, O, C, mode, rps)
    call_crop(lib, p_s, bufs_s, B, O, C, rps, row0)
    # fused
    p_f, s_f, g_f, t_f = fresh()
    ring_f, (rp, ctr, cur) = ring_of(entries, 3, 4, 1)
    geom = L().MmtGeomArgs(P(s_f), factor, ring_f if use_ring else L().MmtRingArgs(), use_ring, P(g_f), P(t_f), Lz, Lx)
    bufs_f = crop_buffers(B, O, C, mode, rps)
    call_crop(lib, p_f, bufs_f, B, O, C, rps, row0, geom=geom)
    if use_ring:
        assert keep_s[1].item() == 2 and keep_s[2].item() == 1       # geometry_kernel advanced its counter
        assert ctr.item() == 1 and cur.item() == 1                   # the fused crop did not
    else:
        assert ctr.item() == 1 and cur.item() == -7
    assert torch.equal(p_f, p_s), "params"
    assert torch.equal(s_f, s_s), "state (rf, err)"
    assert torch.equal(g_f, g_s) and torch.equal(t_f, t_s)
    assert g_f[-1].item() == -7 and t_f[-1].item() == -7
    for k in bufs_s:
        assert (bufs_s[k] is None and bufs_f[k] is None) or torch.equal(bufs_f[k], bufs_s[k]), k
    # and both are the oracle's crop of the box
    st = from_dev(s_f, L().MmtSeqState, B)
    assert [s.err for s in st] == [0, E_BOX, 0]
    expected = []
    for b, box in enumerate(FUSED_BOXES):
        if st[b].err:
            expected.append(crop_expected("big", 0, 0, 1, O))
        else:
            patch, rf = ocrop.sample_target(frame("big"), list(box), factor, O)
            assert dbits(st[b].rf) == dbits(rf)
            expected.append((patch, tokens_of(patch)))
    check_crop(bufs_f, expected, O, C, mode, rps, row0)


# ------------------------------------------------------------------------------------------ decode
BR_OF = [0, 1, 1, 2, 2]
CLAMP_LO = float(np.float32(1e-4))
CLAMP_HI = float(np.float32(1) - np.float32(1e-4))


def decode_inputs(fs, B, seed, ctr_scale=0.5):
    """Random non-negative h4 [3][B][n][32] (different per sequence and branch plane), random w5 / b5."""
    g = torch.Generator().manual_seed(seed)
    n = fs * fs
    h4 = torch.rand(3, B, n, 32, generator=g) * torch.rand(3, B, 1, 1, generator=g).add(0.5)
    w5 = torch.randn(5, 32, generator=g) * torch.tensor([ctr_scale, 0.1, 0.1, 0.3, 0.3])[:, None]
    b5 = torch.randn(5, generator=g) * 0.2
    return h4.contiguous(), w5.contiguous(), b5, ov.hann2d(fs).reshape(-1).contiguous().float()


def decode_reference(h4, w5, b5, hann):
    """float64 maps [B][5][n] (ctr, size w, size h, offset x, offset y), their bars, the response and its bar."""
    H, Wt, bb = h4.double(), w5.double(), b5.double()
    acc = [H[BR_OF[o]] @ Wt[o] + bb[o] for o in range(5)]
    bar = [(32 + 2) * U * (H[BR_OF[o]].abs() @ Wt[o].abs() + bb[o].abs()) for o in range(5)]

    def sig(a):
        return torch.sigmoid(a).clamp(CLAMP_LO, CLAMP_HI)

    maps = torch.stack([sig(acc[0]), sig(acc[3]), sig(acc[4]), acc[1], acc[2]], 1)
    bars = torch.stack([bar[0] / 4 + 4 * U, bar[3] / 4 + 4 * U, bar[4] / 4 + 4 * U, bar[1], bar[2]], 1)
    resp = hann.double() * maps[:, 0]
    resp_bar = hann.double() * bars[:, 0] + U * resp
    return maps, bars, resp, resp_bar


def argmax_margin(resp, resp_bar):
    """Per sequence: (reference index, top-two margin / (2 * the largest response bar))."""
    out = []
    for b in range(resp.shape[0]):
        top = torch.topk(resp[b], 2)
        out.append((int(top.indices[0]), ((top.values[0] - top.values[1]) / (2 * resp_bar[b].max())).item()))
    return out


def run_decode(lib, h4, w5, b5, hann, fs, maps=True, state_t=None, params_t=None, out_t=None, search_size=256,
               ring_outs=None, ring_cur=None, ring_pitch=0, row0=0, ring_ctr=None, kring=0, expect=0, B=None):
    """decode_kernel; returns (res [B][8], maps [B][5][n] or None) with their guards checked."""
    B = h4.shape[1] if B is None else B
    n = fs * fs
    dev = [t.cuda() for t in (h4, w5, b5, hann)]
    res = torch.full((B + 1, 8), float("nan"), device="cuda")
    mp = torch.full((B * 5 * n + n,), float("nan"), device="cuda") if maps else None
    a = L().MmtDecodeArgs(B, fs, P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(res), P(mp), P(state_t), P(params_t),
                          P(out_t), search_size, P(ring_outs), P(ring_cur), ring_pitch, row0, P(ring_ctr), kring)
    rc = lib.mmt_op_decode(ctypes.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == expect, rc
    if expect:
        assert torch.isnan(res).all() and (mp is None or torch.isnan(mp).all())
        return None, None
    assert torch.isnan(res[B]).all() and not torch.isnan(res[:B]).any(), "res: guard row / unwritten row"
    if maps:
        assert torch.isnan(mp[B * 5 * n:]).all() and not torch.isnan(mp[:B * 5 * n]).any(), "maps: guard / unwritten"
        mp = mp[:B * 5 * n].reshape(B, 5, n).cpu()
    return res[:B].cpu(), mp


def check_gather(res, mp, hann, fs, idx):
    """The result rows against the launch's own maps at the given index, bitwise in float32."""
    for b in range(res.shape[0]):
        p = idx[b]
        r, m = res[b].numpy(), mp[b].numpy()
        assert r[5] == p, (b, r[5], p)
        iy, ix = divmod(p, fs)
        f = np.float32
        assert r[4].tobytes() == (hann.numpy()[p] * m[0, p]).astype(f).tobytes(), "score"
        assert r[0].tobytes() == ((f(ix) + m[3, p]) / f(fs)).astype(f).tobytes(), "cx"
        assert r[1].tobytes() == ((f(iy) + m[4, p]) / f(fs)).astype(f).tobytes(), "cy"
        assert r[2].tobytes() == m[1, p].tobytes() and r[3].tobytes() == m[2, p].tobytes(), "size"
        assert r[6] == 0 and r[7] == 0


DECODE_CASES = [(fs, B) for fs in (3, 16, 17, 24) for B in (1, 3)]


@gpu
@pytest.mark.parametrize("fs,B", DECODE_CASES)
def test_decode_values_and_argmax(lib, fs, B):
    """n = 9 (idle threads), 256, 289 and 576 (the strided loop), B = 1 and 3 with different data per sequence and per
    branch plane (the {0, 1, 1, 2, 2} plane of each output): the five maps against float64, the argmax index, and the
    result row gathered bitwise from the launch's own maps."""
    h4, w5, b5, hann = decode_inputs(fs, B, 100 * fs + B)
    maps, bars, resp, resp_bar = decode_reference(h4, w5, b5, hann)
    ref = argmax_margin(resp, resp_bar)
    assert all(m > 1 for _, m in ref), f"the case's top-two margin is inside twice the response bar: {ref}"
    res, mp = run_decode(lib, h4, w5, b5, hann, fs)
    ratio = ((mp.double() - maps).abs() / bars).amax(dim=(0, 2))
    print(f"decode fs={fs} B={B}: worst |err| / bar ctr {ratio[0]:.3f} size {max(ratio[1], ratio[2]):.3f} "
          f"offset {max(ratio[3], ratio[4]):.3f}; argmax margin / (2 bar) {min(m for _, m in ref):.1f}")
    assert (ratio <= 1).all(), ratio
    check_gather(res, mp, hann, fs, [i for i, _ in ref])


@gpu
@pytest.mark.parametrize("sign", [1, -1])
def test_decode_clamp_ends(lib, sign):
    """b5 = +-30 on the ctr and size outputs: exactly float32(1e-4) and float32(1) - float32(1e-4) (bits 1065351538,
    torch's 1 - 1e-4 in float32); the index is the first occurrence of the largest fp32 product."""
    fs, B = 16, 2
    assert np.float32(CLAMP_HI).view(np.int32) == 1065351538
    h4, w5, b5, hann = decode_inputs(fs, B, 7, ctr_scale=0.05)
    w5 = w5 * 0.2
    b5 = torch.tensor([30.0 * sign, 0.1, -0.2, 30.0 * sign, -30.0 * sign])
    res, mp = run_decode(lib, h4, w5, b5, hann, fs)
    hi, lo = np.float32(CLAMP_HI), np.float32(CLAMP_LO)
    want = (hi, hi, lo) if sign > 0 else (lo, lo, hi)
    for k in range(3):
        assert (mp[:, k].numpy() == want[k]).all(), k
    prod = hann.numpy()[None] * mp[:, 0].numpy()
    check_gather(res, mp, hann, fs, [int(np.argmax(prod[b])) for b in range(B)])


def tie_inputs(fs, sets, seed):
    """One sequence per winner set: every h4 ctr row zero (ctr = sigmoid(-8) there) but the set's rows, which hold one
    common row (None: every position holds it)."""
    g = torch.Generator().manual_seed(seed)
    B, n = len(sets), fs * fs
    h4 = torch.rand(3, B, n, 32, generator=g)
    h4[0] = 0
    row = torch.rand(32, generator=g) + 0.1
    for b, s in enumerate(sets):
        if s is None:
            h4[0, b] = row
        else:
            h4[0, b, list(s)] = row
    w5 = torch.randn(5, 32, generator=g) * 0.1
    w5[0] = (torch.rand(32, generator=g) + 0.2) * 0.8      # sum row * w ~ 10: ctr ~ sigmoid(2) on the set
    b5 = torch.tensor([-8.0, 0.1, -0.1, 0.2, -0.3])
    return h4, w5, b5


def tie_sets(fs):
    n = fs * fs
    sets = [None, (n - 2, n - 1)]
    if n > 261:
        sets.append((5, 261))         # one thread's strided loop
    if n > 200:
        sets += [(130, 131), (63, 200)]
    return sets


@gpu
@pytest.mark.parametrize("window", ["ones", "hann"])
@pytest.mark.parametrize("fs", [3, 16, 17, 24])
def test_decode_argmax_ties(lib, fs, window):
    """Exact ties go to the lowest index: inside one thread's strided loop ({5, 261}), between neighbouring threads,
    across the LDS reduction ({63, 200}), in the last two cells, and everywhere at once (index 0).  With the real Hann
    window the sets are those whose members the window weighs bitwise equally (the issue's sets are not symmetric under
    it and drop out; transposed pairs (r, c) / (c, r) are)."""
    n = fs * fs
    if window == "ones":
        hann, sets = torch.ones(n), tie_sets(fs)
    else:
        hann = ov.hann2d(fs).reshape(-1).contiguous().float()
        cand = tie_sets(fs)[1:] + [(fs + 2, 2 * fs + 1)] + ([(5, 5 * fs)] if fs > 5 else [])
        if n > 261:   # cell 261 and its transpose: two threads, one of them in its second pass
            cand.append((261 % fs * fs + 261 // fs, 261))
        sets = [s for s in cand if len(set(s)) == 2 and len({hann[p].item() for p in s}) == 1]
        assert sets, "transposed pairs are weighed equally: the product of the same two factors"
        sets = [tuple(sorted(s)) for s in sets]
    h4, w5, b5 = tie_inputs(fs, sets, fs)
    res, mp = run_decode(lib, h4, w5, b5, hann, fs)
    prod = hann.numpy()[None] * mp[:, 0].numpy()                  # fp32, as the kernel forms it
    want = []
    for b, s in enumerate(sets):
        members = list(range(n)) if s is None else list(s)
        top = prod[b].max()
        assert sorted(np.flatnonzero(prod[b] == top).tolist()) == sorted(members), "the case is not the tie it means"
        want.append(min(members))
    assert want[0] == 0 or window == "hann"
    check_gather(res, mp, hann, fs, want)


# ---- state update
def state_reference(res4, search_size, rf, state_box, H, W):
    """oracle/tracker.py: pred_box through float32 tensors, then map_box_back and clip_box in python floats."""
    pred_box = (torch.tensor(res4) * search_size / rf).tolist()
    t = otracker.OracleTracker.__new__(otracker.OracleTracker)
    t.state, t.cfg = list(state_box), ov.NetCfg(search_size=search_size)
    raw = t.map_box_back(pred_box, rf)
    return otracker.clip_box(raw, H, W, margin=10), raw


# name, previous box, crop_sz, (cx, cy, w, h) of the prediction in crop units, frame (H, W), the clip it must take
STATE_CASES = [
    ("interior", (300.0, 220.0, 40.0, 40.0), 200, (0.55, 0.45, 0.2, 0.15), (480, 640), None),
    ("x1<0", (10.0, 220.0, 40.0, 40.0), 200, (0.4, 0.5, 0.3, 0.2), (480, 640), lambda r, H, W: r[0] < 0),
    ("x1>W-10", (610.0, 220.0, 40.0, 40.0), 200, (0.6, 0.5, 0.05, 0.2), (480, 640), lambda r, H, W: r[0] > W - 10),
    ("x2<10", (-10.0, 220.0, 40.0, 40.0), 200, (0.4, 0.5, 0.1, 0.2), (480, 640), lambda r, H, W: r[0] + r[2] < 10),
    ("x2>W", (580.0, 220.0, 40.0, 40.0), 200, (0.6, 0.5, 0.3, 0.2), (480, 640),
     lambda r, H, W: r[0] + r[2] > W and r[0] < W - 10),
    ("y1<0", (300.0, 10.0, 40.0, 40.0), 200, (0.5, 0.4, 0.2, 0.3), (480, 640), lambda r, H, W: r[1] < 0),
    ("y1>H-10", (300.0, 450.0, 40.0, 40.0), 200, (0.5, 0.6, 0.2, 0.05), (480, 640), lambda r, H, W: r[1] > H - 10),
    ("y2<10", (300.0, -10.0, 40.0, 40.0), 200, (0.5, 0.4, 0.2, 0.1), (480, 640), lambda r, H, W: r[1] + r[3] < 10),
    ("y2>H", (300.0, 420.0, 40.0, 40.0), 200, (0.5, 0.6, 0.2, 0.3), (480, 640),
     lambda r, H, W: r[1] + r[3] > H and r[1] < H - 10),
    ("w,h<margin", (300.0, 220.0, 40.0, 40.0), 200, (0.5, 0.5, 0.01, 0.02), (480, 640),
     lambda r, H, W: r[2] < 10 and r[3] < 10),
    ("spans", (300.0, 220.0, 40.0, 40.0), 1000, (0.5, 0.5, 0.9, 0.8), (481, 637),
     lambda r, H, W: r[0] < 0 and r[1] < 0 and r[0] + r[2] > W and r[1] + r[3] > H),
    ("rf 256/173", (300.3, 220.7, 41.1, 39.9), 173, (0.47, 0.58, 0.31, 0.22), (480, 640), None),
]


def unclipped(r, H, W):
    return 0 <= r[0] <= W - 10 and 10 <= r[0] + r[2] <= W and 0 <= r[1] <= H - 10 and 10 <= r[1] + r[3] <= H and \
        r[2] >= 10 and r[3] >= 10


def state_inputs(pred, fs):
    """Zero conv5 weights but one ctr weight: the offset and size maps are the constants of b5, and the one boosted
    ctr row (cell p of both sequences) makes p the argmax -- so the test decides cx, cy, w, h."""
    cx, cy, w, h = pred
    n = fs * fs
    ix, iy = int(cx * fs), int(cy * fs)
    p = iy * fs + ix
    h4 = torch.zeros(3, 2, n, 32)
    h4[0, :, p, 0] = 1.0
    w5 = torch.zeros(5, 32)
    w5[0, 0] = 20.0
    b5 = torch.tensor([-10.0, cx * fs - ix, cy * fs - iy, math.log(w / (1 - w)), math.log(h / (1 - h))])
    return h4, w5, b5, p


@gpu
@pytest.mark.parametrize("search_size,fs", [(256, 16), (384, 24)])
def test_decode_state_update(lib, search_size, fs):
    """The box mapped back and clipped, as doubles: every clip_box branch, sizes below the margin, a box spanning the
    frame, a non-power-of-two rf.  One launch per case, of two sequences: the case, and the same state with
    state.err = -5, which keeps its state and still reports the score."""
    hann = ov.hann2d(fs).reshape(-1).contiguous().float()
    for name, box, cs, pred, (H, W), branch in STATE_CASES:
        h4, w5, b5, p = state_inputs(pred, fs)
        rf = search_size / cs
        states = [seq_state(box, rf, 0), seq_state(box, rf, E_BOX)]
        params = [L().MmtCropParam(None, 0, H, W, 6, -1, -1, cs, 0)] * 2
        state_t, params_t = to_dev(states, L().MmtSeqState), to_dev(params, L().MmtCropParam)
        out_t = sentinel(L().MmtTrackOut, 3)
        res, mp = run_decode(lib, h4, w5, b5, hann, fs, state_t=state_t, params_t=params_t, out_t=out_t,
                             search_size=search_size)
        check_gather(res, mp, hann, fs, [p, p])
        guard_ok(out_t, L().MmtTrackOut, 2, "out")
        guard_ok(state_t, L().MmtSeqState, 2, "state")
        assert bytes(params_t.cpu().numpy()[:2 * 48]) == b"".join(bytes(q) for q in params), "params are read only"
        outs, sts = from_dev(out_t, L().MmtTrackOut, 2), from_dev(state_t, L().MmtSeqState, 2)
        for b in range(2):
            assert np.float32(outs[b].score).tobytes() == res[b, 4].numpy().tobytes(), name
        # the error sequence
        assert outs[1].err == E_BOX and [dbits(v) for v in outs[1].box] == [dbits(v) for v in box], name
        assert bytes(sts[1]) == bytes(states[1]), f"{name}: an error sequence's state changed"
        # the case
        want, raw = state_reference(res[0, :4].tolist(), search_size, rf, box, H, W)
        if branch is not None:
            assert branch(raw, H, W), f"{name}: the case does not take the clip it is named for ({raw})"
        else:
            assert unclipped(raw, H, W), f"{name}: meant to be unclipped ({raw})"
        assert outs[0].err == 0
        assert [dbits(v) for v in outs[0].box] == [dbits(float(v)) for v in want], (name, list(outs[0].box), want)
        assert [dbits(v) for v in sts[0].box] == [dbits(float(v)) for v in want], name
        assert dbits(sts[0].rf) == dbits(rf) and sts[0].err == 0


@gpu
@pytest.mark.parametrize("cur0,with_ctr", [(0, True), (1, True), (2, True), (1, False)])
def test_decode_ring(lib, cur0, with_ctr):
    """ring_pitch = 4, row0 = 1, B = 2 over kring = 3: the two records land at cur * pitch + 1 + b and nowhere else;
    ring_ctr becomes cur + 1 (0 after the last entry), and is left alone when not passed."""
    fs, B, kring, pitch = 3, 2, 3, 4
    h4, w5, b5, hann = decode_inputs(fs, B, 11)
    states = [seq_state((100.0, 80.0, 30.0, 20.0), 256 / 120, 0), seq_state((50.0, 60.0, 20.0, 30.0), 256 / 90, 0)]
    params = [L().MmtCropParam(None, 0, 300, 400, 6, 0, 0, 120, 0), L().MmtCropParam(None, 0, 300, 400, 6, 0, 0, 90, 0)]
    state_t, params_t = to_dev(states, L().MmtSeqState), to_dev(params, L().MmtCropParam)
    out_t, ring_t = sentinel(L().MmtTrackOut, B + 1), sentinel(L().MmtTrackOut, kring * pitch + 1)
    cur, ctr = ints([cur0]), ints([-7])
    run_decode(lib, h4, w5, b5, hann, fs, state_t=state_t, params_t=params_t, out_t=out_t, ring_outs=ring_t,
               ring_cur=cur, ring_pitch=pitch, row0=1, ring_ctr=ctr if with_ctr else None, kring=kring)
    assert cur.item() == cur0
    assert ctr.item() == ((cur0 + 1) % kring if with_ctr else -7)
    sz = ctypes.sizeof(L().MmtTrackOut)
    ring, out = ring_t.cpu().numpy(), out_t.cpu().numpy()
    first = (cur0 * pitch + 1) * sz
    assert (ring[:first] == FILL8).all() and (ring[first + B * sz:] == FILL8).all(), "a record outside the entry"
    assert bytes(ring[first:first + B * sz]) == bytes(out[:B * sz])
    assert (out[:B * sz] != FILL8).any() and (out[B * sz:] == FILL8).all()


@gpu
def test_decode_rejects(lib):
    fs, B = 3, 2
    h4, w5, b5, hann = decode_inputs(fs, B, 3)
    st = to_dev([seq_state((1.0, 2.0, 30.0, 40.0), 1.0, 0)] * B, L().MmtSeqState)
    pr = to_dev([L().MmtCropParam(None, 0, 300, 400, 6, 0, 0, 120, 0)] * B, L().MmtCropParam)
    out, ring = sentinel(L().MmtTrackOut, B + 1), sentinel(L().MmtTrackOut, 13)
    keep = [t.clone() for t in (st, pr)]
    cur, ctr = ints([0]), ints([-7])
    full = dict(state_t=st, params_t=pr, out_t=out, ring_outs=ring, ring_cur=cur, ring_pitch=4, row0=1, ring_ctr=ctr,
                kring=3)
    run_decode(lib, h4, w5, b5, hann, 0, expect=E_ARG, B=B)                       # fs < 1
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, B=0)                      # B < 1
    for drop in ("params_t", "out_t", "ring_cur"):
        run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, drop: None})
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, "search_size": 0})
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, "row0": 3})    # row0 + B > pitch
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, "kring": 0})
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, "ring_cur": ints([3])})   # entry outside the ring
    run_decode(lib, h4, w5, b5, hann, fs, expect=E_ARG, **{**full, "state_t": None})         # a ring without a state
    dev = [t.cuda() for t in (h4, w5, b5, hann)] + [torch.full((B + 1, 8), float("nan"), device="cuda")]
    for null in range(5):                                                         # each required pointer
        ptrs = [None if i == null else P(t) for i, t in enumerate(dev)]
        a = L().MmtDecodeArgs(B, fs, *ptrs, None)
        assert lib.mmt_op_decode(ctypes.byref(a), _stream()) == E_ARG, null
    torch.cuda.synchronize()
    assert torch.isnan(dev[4]).all()
    assert lib.mmt_op_decode(None, _stream()) == E_ARG
    torch.cuda.synchronize()
    assert torch.equal(st, keep[0]) and torch.equal(pr, keep[1])
    assert (out == FILL8).all() and (ring == FILL8).all() and ctr.item() == -7 and cur.item() == 0
