"""The GEMM launch forms of the engine that no other operator test reaches, through mmt_op_gemm_ex (GPU only).

mmt_op_gemm / mmt_op_gemm_f16x3 launch one group, alone on the chip, into the library's own workspace.  The engine
(csrc/engine_forward.cpp) also launches

* the head's 3 x 3 convs in the default f16x3 precision: conv1 (K = 6912) on the 128 x 192 / 128 x 128 tiles; conv2,
  conv3, conv4 as three groups per launch, conv2 reading column slices of conv1's output (lda = 3 hc, conv_cin = hc),
  conv4 writing ReLU fp32 through the 64 x 32 / 32 x 32 tiles (head.py:8-21, 45-62);
* the same convs at one sequence as split-K launches with uneven K slices and the per-group reduce launch;
* the two-group patch embedding (patch_embed.py:20, its own inv per group) and OSTrack's position epilogue with
  pos_rows > 1 on gemm_kernel, gemm128w and gemm256s;
* the residual GEMMs of a small launch with defer_reduce: the raw split-K slabs stay in the workspace and the next
  token kernel combines them (kernels.h RowReduce), bit for bit "the arithmetic of the reduce launch it replaces".

Operands and tolerances follow test_gpu_f16x3.py: random fp32 operands split at power-of-two range scales, the
reference in float64 on the reconstructed (hi + lo) / s operands, max|out - y| <= 1e-5 max|y| (+ 4e-7 max|R + y| for
the residual epilogues); the bf16 cases hold test_gemm_conv3x3's rtol 1e-2 / atol 2e-2 on bf16-rounded operands.
On these operands a dropped Wl*Ah or Wh*Al term moves the outputs by about 5e-4 (twenty times the bar at K = 576 and at
K = 6912 alike) and a lost conv tap by about 0.7.  Every group of a launch has its own operands, bias and magnitude (x1, x3, x0.2), so its inv and out_scale differ from
its neighbours' and a mixed-up group fails.  The conv reference is nine shifted float64 matmuls over the zero-padded
NHWC map, weights [out][ky][kx][in]; a few whole pixel rows of every conv input are zero (hi = lo = 0), as
final_norm_recover leaves pruned slots.  Every case asserts the tile and K slices the launch reports: the tables
below are the rules' choices at the MI355X's 256 CUs (tests/gemm_plan_print), so a planner change cannot silently move
a case to another kernel.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 768
WS_ELEMS = 4 << 20      # the engine's split-K workspace per launch part (engine.h kSplitKWsElems), in floats
WS_TAIL = 4096          # floats past it that no launch may touch
A_MAG = (1.0, 3.0, 0.2)
W_MAG = (1.0, 0.5, 2.0)


@pytest.fixture(scope="module")
def lib():
    from mmtrack_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ws():
    return torch.full((WS_ELEMS + WS_TAIL,), float("nan"), device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def need_256_cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    if n != 256:
        pytest.skip(f"the expected tiles are the rules' choices at 256 CUs; this device reports {n}")


def range_scale(t):
    """engine_weights.cpp range_scale: the power of two s with max|t| * s <= 2^14."""
    m = float(t.abs().max())
    return 2.0 ** (14 - math.ceil(math.log2(m))) if m > 0 else 1.0


def split(t, s):
    """fp16 hi / lo halves of t * s (fp32 arithmetic, RNE) and the exact value they carry, in float64."""
    v = t.float() * s
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.contiguous(), lo.contiguous(), (hi.double() + lo.double()) / s


def nan_rows(rows, cols, dtype=torch.float32):
    """rows + 1 NaN rows: the outputs of a launch and one guard row after them."""
    return torch.full((rows + 1, cols), float("nan"), device="cuda", dtype=dtype)


def check_guard(t, rows, what):
    assert torch.isnan(t[rows].float()).all(), f"{what}: a store past the last row"
    assert not torch.isnan(t[:rows].float()).any(), f"{what}: NaN within the M rows"


def P(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def launch(lib, groups, M, N, K, epi, split_mode, conv_hw=0, conv_cin=0, pos_rows=0, conc=0, defer=0, ws=None,
           ws_elems=0):
    """mmt_op_gemm_ex over `groups` (dicts of mmt_gemm_group's fields, pointers as integers) -> (tile, ksplit,
    deferred) as the launch reported them."""
    from mmtrack_amd import _lib
    a = _lib.MmtGemmExArgs()
    for k, g in enumerate(groups):
        for name, v in g.items():
            setattr(a.g[k], name, v)
    a.groups, a.M, a.N, a.K, a.epi, a.split = len(groups), M, N, K, epi, split_mode
    a.conv_hw, a.conv_cin, a.pos_rows, a.conc, a.defer_reduce = conv_hw, conv_cin, pos_rows, conc, defer
    a.ws, a.ws_elems = P(ws), ws_elems
    ran = _lib.MmtGemmRan()
    rc = lib.mmt_op_gemm_ex(ctypes.byref(a), ctypes.byref(ran), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ran.tile.decode(), ran.ksplit, ran.deferred


def operand(gen, rows, cols, mag, zero_rows=None):
    t = torch.randn(rows, cols, device="cuda", generator=gen) * mag
    if zero_rows is not None:
        t[zero_rows] = 0.0
    return t


def weights(gen, N, K, mag):
    return torch.randn(N, K, device="cuda", generator=gen) * (0.5 / math.sqrt(K) * mag)


def with_guard_row(t):
    """t with one zero row appended (a conv A resource spans M rows of lda from a column-offset base)."""
    return torch.cat([t, torch.zeros_like(t[:1])]).contiguous()


def conv3x3_ref(x64, w64, bias, maps, hw, cin):
    """head.py:8-21 conv3x3 (pad 1) + ReLU as nine shifted float64 matmuls; x64 [maps * hw * hw][cin] NHWC rows,
    w64 [out][ky][kx][in]."""
    xp = torch.zeros(maps, hw + 2, hw + 2, cin, device="cuda", dtype=torch.float64)
    xp[:, 1:hw + 1, 1:hw + 1] = x64.view(maps, hw, hw, cin)
    w = w64.view(-1, 3, 3, cin)
    ref = bias.double().expand(maps * hw * hw, -1).clone()
    for ky in range(3):
        for kx in range(3):
            ref += xp[:, ky:ky + hw, kx:kx + hw].reshape(maps * hw * hw, cin) @ w[:, ky, kx].t()
    return torch.relu(ref), ref


def zero_pixels(gen, maps, hw):
    """a few whole pixel rows per map: the first and the last pixel of the launch, and random ones (borders included)"""
    plane = hw * hw
    idx = torch.randint(0, plane, (maps, 4), device="cuda", generator=gen) + torch.arange(maps, device="cuda")[:, None] * plane
    return torch.cat([idx.reshape(-1), torch.tensor([0, hw - 1, maps * plane - 1], device="cuda")])


# launch: cin, cout, epilogue (head.py CenterPredictor: 768 -> 256 x 3 -> 128 -> 64 -> 32 per branch)
CONV = {"conv1": (768, 768, 3), "conv2": (256, 128, 3), "conv3": (128, 64, 3), "conv4": (64, 32, 5)}

CONV_F16X3 = [
    # launch, M, hw, conc, tile, K slices
    ("conv1", 4096, 16, 2, "128x192_4x2_s2_k64", 1),   # 2 x 16 sequences
    ("conv1", 1728, 24, 0, "128x128_4x2_s2_k64", 1),   # OSTrack-384, M % 128 = 64, tiles straddle maps
    ("conv1", 256, 16, 0, "64x64_4x2_s3_k64", 5),      # one sequence: 108 K-tiles in 5 slices
    ("conv2", 2880, 24, 0, "128x128_4x2_s2_k64", 1),
    ("conv2", 1728, 24, 0, "64x64_4x2_s3_k64", 1),
    ("conv2", 256, 16, 0, "64x64_4x2_s3_k64", 8),      # 36 K-tiles in 8 slices
    ("conv3", 9216, 24, 2, "128x64_2x2_s2_k64", 1),
    ("conv3", 1728, 24, 0, "64x64_4x2_s3_k64", 3),
    ("conv3", 256, 16, 0, "64x64_4x2_s3_k64", 4),      # 18 K-tiles in 4 slices
    ("conv4", 9216, 24, 2, "64x32_4x1_s2_k64", 1),
    ("conv4", 1728, 24, 0, "32x32_2x1_s2_k64", 1),
]
CONV_BF16 = [
    ("conv2", 8192, 16, 0, "128x64_2x2_s2_k64", 1),
    ("conv3", 8192, 16, 0, "64x64_4x2_s4_k64", 1),
    ("conv4", 8192, 16, 0, "64x32_4x1_s2_k64", 1),
    ("conv2", 1728, 24, 0, "64x64_4x2_s4_k64", 1),
    ("conv4", 1728, 24, 0, "32x32_2x1_s2_k64", 1),
]


def conv_case(lib, ws, name, M, hw, conc, tile, ks, f16x3):
    """One head conv launch as head() (engine_forward.cpp) issues it; conv1 is one group of N = 3 hc, the others three
    groups writing per-branch planes (ldc = cout), conv2 reading its A from column slices of one [M][768] buffer."""
    need_256_cus()
    cin, co, epi = CONV[name]
    G = 1 if name == "conv1" else 3
    K, maps = 9 * cin, M // (hw * hw)
    assert maps * hw * hw == M
    gen = torch.Generator(device="cuda").manual_seed(M + 7 * co + hw + (0 if f16x3 else 1))
    zr = zero_pixels(gen, maps, hw)
    shared = name == "conv2"   # one buffer, group k at column offset cin * k, lda = 3 * cin
    lda = G * cin if shared else cin
    adt = torch.float16 if f16x3 else torch.bfloat16
    Ah = torch.zeros(M + 1, lda, device="cuda", dtype=adt)
    Al = torch.zeros_like(Ah) if f16x3 else None
    groups, keep, refs = [], [], []
    for k in range(G):
        A = operand(gen, M, cin, A_MAG[k], zr)
        W = weights(gen, co, K, W_MAG[k])
        bias = torch.randn(co, device="cuda", generator=gen) * (0.1 * A_MAG[k] * W_MAG[k])
        c0 = k * cin if shared else 0
        if not shared and k:
            Ah, Al = torch.zeros_like(Ah), (torch.zeros_like(Ah) if f16x3 else None)
        if f16x3:
            sa, sw = range_scale(A), range_scale(W)
            hi, lo, A64 = split(A, sa)
            Wh, Wl, W64 = split(W, sw)
            Ah[:M, c0:c0 + cin], Al[:M, c0:c0 + cin] = hi, lo
            assert not Ah[zr, c0:c0 + cin].any() and not Al[zr, c0:c0 + cin].any()
            inv = 1.0 / (sa * sw)
        else:
            Ab, Wh, Wl = A.bfloat16(), W.bfloat16().contiguous(), None
            Ah[:M, c0:c0 + cin] = Ab
            A64, W64, inv = Ab.double(), Wh.double(), 1.0
        y, ref = conv3x3_ref(A64, W64, bias, maps, hw, cin)
        so = range_scale(y.float()) if (f16x3 and epi == 3) else 1.0
        odt = torch.float32 if epi == 5 else adt
        Cc = nan_rows(M, co, odt)
        Cl = nan_rows(M, co, odt) if (f16x3 and epi == 3) else None
        groups.append(dict(A=P(Ah, c0), A_lo=P(Al, c0), lda=lda, W=P(Wh), W_lo=P(Wl), ldw=K, bias=P(bias), C=P(Cc),
                           C_lo=P(Cl), ldc=co, R=None, ldr=0, inv=inv, out_scale=so))
        keep.append((Ah, Al, Wh, Wl, bias))
        refs.append((y, ref, Cc, Cl, so))
    got = launch(lib, groups, M, co, K, epi, 1 if f16x3 else 0, conv_hw=hw, conv_cin=cin, conc=conc,
                 ws=ws if f16x3 else None, ws_elems=WS_ELEMS if f16x3 else 0)
    assert got == (tile, ks, 0), got
    for k, (y, ref, Cc, Cl, so) in enumerate(refs):
        what = f"{'f16x3' if f16x3 else 'bf16'} {name} M={M} hw={hw} group {k}"
        check_guard(Cc, M, what)
        out = Cc[:M].double()
        if Cl is not None:
            check_guard(Cl, M, what + " (lo)")
            out = (out + Cl[:M].double()) / so
        err = (out - y).abs()
        if f16x3:
            tol = torch.full_like(y, 1e-5 * float(y.abs().max()))
        else:
            tol = 2e-2 + 1e-2 * y.abs()
        print(f"{what} [{tile} ks={ks}]: max|err| {float(err.max()):.3e} (tol {float(tol.max()):.3e}, "
              f"max|y| {float(y.abs().max()):.3e})")
        assert (err <= tol).all(), what
        off = ref < -tol   # ReLU: exact zeros in both halves
        assert bool(off.any())
        assert (Cc[:M][off] == 0).all(), what
        assert Cl is None or (Cl[:M][off] == 0).all(), what


@pytest.mark.parametrize("name,M,hw,conc,tile,ks", CONV_F16X3, ids=[f"{c[0]}-M{c[1]}" for c in CONV_F16X3])
def test_head_conv_f16x3(lib, ws, name, M, hw, conc, tile, ks):
    """The head convs in the default precision against float64, per group, at 1e-5 of the output scale: the tiles of
    the 2 x 16 sequence launch and OSTrack-384, and one sequence's split-K launches with the per-group reduce."""
    conv_case(lib, ws, name, M, hw, conc, tile, ks, True)


@pytest.mark.parametrize("name,M,hw,conc,tile,ks", CONV_BF16, ids=[f"{c[0]}-M{c[1]}" for c in CONV_BF16])
def test_head_conv_bf16_groups(lib, ws, name, M, hw, conc, tile, ks):
    """The three-group convs in the bf16 mode (split = 0, no workspace), tolerance as test_gemm_conv3x3."""
    conv_case(lib, ws, name, M, hw, conc, tile, ks, False)


PATCH = [
    # M, f16x3, conc, tile
    (5120, True, 2, "128x128_4x2_s2_k64"),   # one stream half of 16 x 320 tokens
    (320, True, 0, "64x64_4x2_s3_k64"),      # one sequence
    (640, False, 0, "64x64_4x2_s4_k64"),     # bf16 mode
]


@pytest.mark.parametrize("M,f16x3,conc,tile", PATCH, ids=[f"M{c[0]}-{'f16x3' if c[1] else 'bf16'}" for c in PATCH])
def test_patch_embed_two_groups(lib, ws, M, f16x3, conc, tile):
    """patch_embed.py:20 for the RGB and the auxiliary modality in one launch (EPI_F32): two groups, each with its own
    weights, bias and inv = 1 / (kPixScale s_W)."""
    need_256_cus()
    gen = torch.Generator(device="cuda").manual_seed(M + (0 if f16x3 else 1))
    groups, keep, refs = [], [], []
    for k in range(2):
        A = operand(gen, M, C, (3.0, 0.2)[k])
        W = weights(gen, C, C, W_MAG[k])
        bias = torch.randn(C, device="cuda", generator=gen) * (0.1, 0.02)[k]
        if f16x3:
            sa, sw = range_scale(A), range_scale(W)
            Ah, Al, A64 = split(A, sa)
            Wh, Wl, W64 = split(W, sw)
            inv = 1.0 / (sa * sw)
        else:
            Ah, Wh, Al, Wl, inv = A.bfloat16(), W.bfloat16(), None, None, 1.0
            A64, W64 = Ah.double(), Wh.double()
        y = A64 @ W64.t() + bias.double()
        Cc = nan_rows(M, C)
        groups.append(dict(A=P(Ah), A_lo=P(Al), lda=C, W=P(Wh), W_lo=P(Wl), ldw=C, bias=P(bias), C=P(Cc), C_lo=None,
                           ldc=C, R=None, ldr=0, inv=inv, out_scale=1.0))
        keep.append((Ah, Al, Wh, Wl, bias))
        refs.append((y, Cc))
    got = launch(lib, groups, M, C, C, 4, 1 if f16x3 else 0, conc=conc, ws=ws if f16x3 else None,
                 ws_elems=WS_ELEMS if f16x3 else 0)
    assert got == (tile, 1, 0), got
    for k, (y, Cc) in enumerate(refs):
        what = f"{'f16x3' if f16x3 else 'bf16'} patch M={M} group {k}"
        check_guard(Cc, M, what)
        err = (Cc[:M].double() - y).abs()
        tol = torch.full_like(y, 1e-5 * float(y.abs().max())) if f16x3 else 2e-2 + 1e-2 * y.abs()
        print(f"{what} [{tile}]: max|err| {float(err.max()):.3e} (tol {float(tol.max()):.3e})")
        assert (err <= tol).all(), what


POS = [
    # M, pos_rows, force, tile
    (1440, 720, -1, "128x128_4x2_s2_k64"),
    (1440, 720, 128, "gemm128w"),
    (1440, 720, 256, "gemm256s"),
    (720, 360, -1, "64x64_4x2_s3_k64"),
]


@pytest.mark.parametrize("M,pos_rows,force,tile", POS, ids=[f"M{c[0]}-{c[3]}" for c in POS])
def test_patch_embed_pos_rows(lib, ws, M, pos_rows, force, tile):
    """OSTrack's patch embedding + pos_embed (EPI_POS_F32, C = acc * inv + bias + R[m % pos_rows]) with two sequences
    of pos_rows tokens, on each of the three kernels that carry the epilogue."""
    need_256_cus()
    gen = torch.Generator(device="cuda").manual_seed(M + pos_rows + force)
    A = operand(gen, M, C, 3.0)
    W = weights(gen, C, C, 1.0)
    bias = torch.randn(C, device="cuda", generator=gen) * 0.1
    R = torch.randn(pos_rows, C, device="cuda", generator=gen)
    sa, sw = range_scale(A), range_scale(W)
    Ah, Al, A64 = split(A, sa)
    Wh, Wl, W64 = split(W, sw)
    ref = A64 @ W64.t() + bias.double()
    y = ref + R.double()[torch.arange(M, device="cuda") % pos_rows]
    Cc = nan_rows(M, C)
    grp = dict(A=P(Ah), A_lo=P(Al), lda=C, W=P(Wh), W_lo=P(Wl), ldw=C, bias=P(bias), C=P(Cc), C_lo=None, ldc=C,
               R=P(R), ldr=C, inv=1.0 / (sa * sw), out_scale=1.0)
    lib.mmt_gemm_force_config(force)
    try:
        got = launch(lib, [grp], M, C, C, 6, 1, pos_rows=pos_rows, ws=ws, ws_elems=WS_ELEMS)
    finally:
        lib.mmt_gemm_force_config(-1)
    assert got == (tile, 1, 0), got
    check_guard(Cc, M, f"patch+pos M={M}")
    err = float((Cc[:M].double() - y).abs().max())
    tol = 1e-5 * float(ref.abs().max()) + 4e-7 * float(y.abs().max())
    print(f"f16x3 patch+pos M={M} pos_rows={pos_rows} [{tile}]: max|err| {err:.3e} (tol {tol:.3e})")
    assert err <= tol


DEFER = [
    # M, K, workspace ("full": the engine's, "small": 500 000 floats, None), conc, tile, K slices, deferred
    (320, 768, "full", 0, "64x64_4x2_s3_k64", 3, 1),      # proj at one sequence
    (320, 3072, "full", 0, "64x64_4x2_s3_k64", 4, 1),     # fc2
    (153, 3072, "full", 0, "64x64_4x2_s3_k64", 7, 1),     # fc2 after the last CE: 48 K-tiles in 7 slices
    (100, 3072, "full", 0, "64x64_4x2_s3_k64", 8, 1),
    (320, 3072, "small", 0, "64x64_4x2_s3_k64", 2, 1),    # the capacity clamp
    (320, 3072, None, 0, "64x64_4x2_s3_k64", 1, 0),       # no workspace: never split
    (5120, 768, "full", 2, "gemm128w", 1, 0),             # a filled launch: nothing to defer
]


def ln_ex(lib, x, w, b, rows, of, xcopy=None, rr=None):
    rc = lib.mmt_op_layernorm_ex(P(x), P(w), P(b), None, None, 1.0, P(of), rows, rows, None, rows, P(xcopy), rr,
                                 _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,K,wsmode,conc,tile,ks,deferred", DEFER,
                         ids=[f"M{c[0]}-K{c[1]}-{c[2]}" for c in DEFER])
def test_resid_gemm_defer_reduce(lib, ws, M, K, wsmode, conc, tile, ks, deferred):
    """proj / fc2 in place on the residual stream with defer_reduce, as run_resid_gemm (engine_forward.cpp) launches
    them: a split-K run leaves X untouched and slabs [ks][M][768] of raw sums (no inv, no bias) at the start of the
    workspace, nothing after them; the consumer's RowReduce over those slabs gives the bits of the reduce launch."""
    from mmtrack_amd import _lib
    need_256_cus()
    gen = torch.Generator(device="cuda").manual_seed(M + K + len(str(wsmode)))
    A = operand(gen, M, K, 1.0)
    W = weights(gen, C, K, 1.0)
    bias = torch.randn(C, device="cuda", generator=gen) * 0.1
    X0 = torch.randn(M, C, device="cuda", generator=gen)
    sa, sw = range_scale(A), range_scale(W)
    Ah, Al, A64 = split(A, sa)
    Wh, Wl, W64 = split(W, sw)
    inv = 1.0 / (sa * sw)
    ref = A64 @ W64.t() + bias.double()
    y = X0.double() + ref
    tol = 1e-5 * float(ref.abs().max()) + 4e-7 * float(y.abs().max())
    w_arg = ws if wsmode else None
    w_elems = {"full": WS_ELEMS, "small": 500000, None: 0}[wsmode]

    def run(defer):
        X = nan_rows(M, C)
        X[:M] = X0
        ws.fill_(float("nan"))
        grp = dict(A=P(Ah), A_lo=P(Al), lda=K, W=P(Wh), W_lo=P(Wl), ldw=K, bias=P(bias), C=P(X), C_lo=None, ldc=C,
                   R=P(X), ldr=C, inv=inv, out_scale=1.0)
        got = launch(lib, [grp], M, C, K, 2, 1, conc=conc, defer=defer, ws=w_arg, ws_elems=w_elems)
        return X, got

    X1, got1 = run(0)    # the reduce launch (or no split): X updated
    assert got1 == (tile, ks, 0), got1
    check_guard(X1, M, "X (defer_reduce = 0)")
    err1 = float((X1[:M].double() - y).abs().max())
    X, got = run(1)
    assert got == (tile, ks, deferred), got
    what = f"f16x3 resid M={M} K={K} ws={wsmode} [{tile} ks={ks} deferred={deferred}]"
    if not deferred:
        check_guard(X, M, "X")
        err = float((X[:M].double() - y).abs().max())
        print(f"{what}: max|err| {err:.3e} (tol {tol:.3e})")
        assert err <= tol and err1 <= tol
        assert torch.equal(X[:M], X1[:M])   # defer_reduce changes nothing where K is not split
        assert torch.isnan(ws).all()        # no slab written
        return
    assert torch.equal(X[:M], X0) and torch.isnan(X[M]).all()          # X untouched
    slabs = ws[:ks * M * C].view(ks, M, C)
    assert not torch.isnan(slabs).any()
    assert torch.isnan(ws[ks * M * C:]).all()                          # nothing past the slabs
    err = float((X0.double() + slabs.double().sum(0) * inv + bias.double() - y).abs().max())
    print(f"{what}: slabs max|err| {err:.3e}, reduce launch {err1:.3e} (tol {tol:.3e})")
    assert err <= tol and err1 <= tol
    # the bitwise contract (kernels.h RowReduce): layernorm_ex applies the pending update and writes X back / to xcopy
    slabs = slabs.clone()
    rr = ctypes.byref(_lib.MmtRowReduce(slabs.data_ptr(), ks, M * C, inv, bias.data_ptr()))
    lw = torch.randn(C, device="cuda", generator=gen) * 0.3 + 1
    lb = torch.randn(C, device="cuda", generator=gen) * 0.2
    of1, ofa, ofb = nan_rows(M, C), nan_rows(M, C), nan_rows(M, C)
    ln_ex(lib, X1, lw, lb, M, of1)
    Xa = X.clone()
    ln_ex(lib, Xa, lw, lb, M, ofa, rr=rr)                               # written back in place
    assert torch.equal(Xa[:M], X1[:M]) and torch.isnan(Xa[M]).all()
    Xb, xc = X.clone(), nan_rows(M, C)
    ln_ex(lib, Xb, lw, lb, M, ofb, xcopy=xc, rr=rr)                     # into xcopy
    assert torch.equal(xc[:M], X1[:M]) and torch.isnan(xc[M]).all()
    assert torch.equal(Xb[:M], X0)                                      # ... and X left as it was
    for of in (of1, ofa, ofb):
        check_guard(of, M, "LN")
    assert torch.equal(ofa[:M], of1[:M]) and torch.equal(ofb[:M], of1[:M])   # LN of the updated row: the same bits
