"""The C-ABI library loads without a GPU and exports every symbol include/mmtrack.h declares."""
import os
import re

from mmtrack_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmtrack.h")


def declared():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmt_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_boundary():
    names = declared()
    for must in ("mmt_create", "mmt_initialize", "mmt_track", "mmt_track_batch", "mmt_set_tensor", "mmt_finalize",
                 "mmt_xcorr", "mmt_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    for name in declared():
        assert hasattr(lib, name), name
    assert set(declared()) == set(_lib.SIGNATURES)


def test_version_without_gpu():
    assert _lib.load().mmt_version().startswith(b"mmtrack-mi355x")


def test_abi_version_matches_header_and_binding():
    """The library, the header's MMT_ABI_VERSION and the ctypes binding agree; the pre-5 strided optimiser
    (stride 0 = contiguous) is not exported, so a binding written against it fails to resolve the symbol."""
    hdr = open(HDR).read()
    v = int(re.search(r"#define\s+MMT_ABI_VERSION\s+(\d+)", hdr).group(1))
    lib = _lib.load()
    assert lib.mmt_abi_version() == v == _lib.ABI_VERSION
    assert not hasattr(lib, "mmt_dimp_optimize_dev")


def test_dimp_state_layout_matches_binding():
    """The device DiMP tracker state / record structs of include/mmtrack.h and the ctypes binding agree in size
    (the library reports sizeof(mmt_dimp_state); no GPU needed)."""
    import ctypes
    from mmtrack_amd import _lib
    lib = _lib.load()
    assert lib.mmt_dimp_state_bytes() == ctypes.sizeof(_lib.MmtDimpState)
    assert _lib.MmtDimpState.target_boxes.offset % 16 == 0 or _lib.MmtDimpState.target_boxes.offset % 4 == 0


def test_frame_op_struct_layouts_match_binding():
    """The structs of the frame-side operator entry points (crop, crop geometry, decode): the size and every field
    offset the library was compiled with equal the ctypes mirror's, field for field (no GPU needed)."""
    import ctypes
    lib = _lib.load()
    for which, cls in enumerate(_lib.STRUCT_LAYOUTS):
        want = [ctypes.sizeof(cls)] + [getattr(cls, name).offset for name, _ in cls._fields_]
        buf = (ctypes.c_size_t * 32)()
        n = lib.mmt_op_struct_layout(which, buf, 32)
        assert n == len(want), cls.__name__
        assert list(buf[:n]) == want, cls.__name__
    assert lib.mmt_op_struct_layout(len(_lib.STRUCT_LAYOUTS), None, 0) == 0
    # the device records are read as arrays: no tail padding surprises
    assert ctypes.sizeof(_lib.MmtCropParam) == 48 and ctypes.sizeof(_lib.MmtSeqState) == 48
    assert ctypes.sizeof(_lib.MmtTrackOut) == 48


def _gemm_ex_args(**over):
    """A valid one-group f16x3 conv launch (conv2's shape) over dummy non-null pointers; `over` replaces fields of the
    launch, or with a g_ prefix of its groups."""
    a = _lib.MmtGemmExArgs()
    a.groups, a.M, a.N, a.K, a.epi, a.split = 1, 256, 128, 2304, 3, 1
    a.conv_hw, a.conv_cin, a.pos_rows, a.conc, a.defer_reduce = 16, 256, 1, 0, 0
    a.ws, a.ws_elems = 0x1000, 1 << 20
    for g in a.g:
        g.A = g.A_lo = g.W = g.W_lo = g.bias = g.C = g.C_lo = g.R = 0x1000
        g.lda, g.ldw, g.ldc, g.ldr, g.inv, g.out_scale = 768, 2304, 128, 128, 1.0, 1.0
    for k, v in over.items():
        if k.startswith("g_"):
            for g in a.g:
                setattr(g, k[2:], v)
        else:
            setattr(a, k, v)
    return a


def test_gemm_ex_rejects_bad_arguments_without_gpu():
    """mmt_op_gemm_ex checks its arguments before any HIP call: every rejected launch below returns MMT_E_ARG over
    dummy pointers on a machine without a GPU (a launch that got past the checks would report MMT_E_HIP or die)."""
    import ctypes
    lib = _lib.load()
    ran = _lib.MmtGemmRan()
    dense = dict(conv_hw=0, conv_cin=0, K=768, N=768)
    bad = [
        dict(groups=0), dict(groups=4), dict(M=0), dict(N=0), dict(K=0), dict(M=-5), dict(K=2304 + 32, conv_hw=0),
        dict(N=48), dict(epi=-1), dict(epi=7),
        dict(g_A=None), dict(g_W=None), dict(g_C=None),
        dict(g_A_lo=None), dict(g_W_lo=None),                  # f16x3 operands without their low halves
        dict(g_C_lo=None),                                     # a split 16-bit epilogue without its low plane
        dict(dense, epi=0, g_C_lo=None), dict(dense, epi=1, g_C_lo=None),
        dict(dense, epi=2, g_R=None), dict(dense, epi=6, g_R=None, pos_rows=4),
        dict(conv_cin=288, K=9 * 288),                         # conv: conv_cin % 64
        dict(conv_cin=128),                                    # conv: K != 9 conv_cin
        dict(epi=0), dict(epi=2), dict(epi=4),                 # conv: not a ReLU epilogue
        dict(g_lda=128),                                       # conv: lda < conv_cin
        dict(ws_elems=-1), dict(ws=None),                      # ws_elems > 0 without a workspace
    ]
    for over in bad:
        a = _gemm_ex_args(**over)
        assert lib.mmt_op_gemm_ex(ctypes.byref(a), ctypes.byref(ran), None) == _lib.MMT_E_ARG, over
        assert lib.mmt_op_gemm_ex(ctypes.byref(a), None, None) == _lib.MMT_E_ARG, over   # a null `ran` is accepted
    assert lib.mmt_op_gemm_ex(None, None, None) == _lib.MMT_E_ARG


def test_conv_launch_plan_without_gpu():
    """The f16x3 conv's host-side launch plan through mmt_conv2d_f16x3_ws_bytes (no GPU call): split-K slices
    follow the output tiles -- the 3 x 3 stride-1 patch kernel tiles 18 x 18 maps over the flattened batch (32 images:
    81 tiles of 128 pixels instead of 96 per-image ones), the generic kernel's 1 x 1 layers fill the chip unsplit."""
    lib = _lib.load()

    def slices(N, H, W, Cin, Cout, k, s, p, G):
        b = lib.mmt_conv2d_f16x3_ws_bytes(N, H, W, Cin, Cout, k, k, s, p, G)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        return b // (G * N * Ho * Wo * Cout * 4) if b else 1

    # layer3 conv2 (2 backbones): 81 tiles x 2 column tiles x 2 = 324 >= 256 slots -> no split (per-image tiles would
    # be 384); the clf conv (one group, 1 024 -> 512, 288 K-tiles: 512 slots): 81 x 4 = 324 -> 3 slices
    assert lib.mmt_conv2d_f16x3_ws_bytes(32, 18, 18, 256, 256, 3, 3, 1, 1, 2) == 0
    assert slices(32, 18, 18, 1024, 512, 3, 1, 1, 1) == 3
    # 4 images: 11 batch tiles (1 296 pixels) x 2 x 2 = 44 -> split K: 5 slices fill 220 of 256 slots
    assert slices(4, 18, 18, 256, 256, 3, 1, 1, 2) == 5
    assert lib.mmt_conv2d_f16x3_ws_bytes(4, 18, 18, 256, 256, 3, 3, 1, 1, 2) == 5 * 2 * 4 * 324 * 256 * 4
    # layer1 conv3 (1 x 1, 72 x 72): 1 296 x 2 x 2 tiles -- no split
    assert lib.mmt_conv2d_f16x3_ws_bytes(32, 72, 72, 64, 256, 1, 1, 1, 0, 2) == 0
    # one image: per-image tiles (3), few tiles -> split over the chunks (at most Cin / 32)
    assert 1 < slices(1, 18, 18, 256, 256, 3, 1, 1, 2) <= 8
    # invalid shapes report no workspace
    assert lib.mmt_conv2d_f16x3_ws_bytes(0, 18, 18, 256, 256, 3, 3, 1, 1, 2) == 0
