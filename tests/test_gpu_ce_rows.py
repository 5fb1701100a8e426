"""The masked template-row CE probability kernel (csrc/ce_rows.hip) through mmt_op_ce_rows / mmt_op_ce_rows_f16x3.

prob[b][h][j] = 1 / nrows[b] * sum_{r in rows[b]} softmax_k(q_r . k_k / 8)[lens_t + j] (attn_blocks.py:44-53 with the
box_mask_z of generate_mask_cond, ce_utils.py:15-65).  The reference is a float64 softmax on the reconstructed
operands, as test_gpu_f16x3.test_attention_f16x3_vs_fp64 (bound 1e-6 on a probability), and fp32 on the bf16 values
for the bf16 kernel, as test_gpu_kernels.test_attention (rtol 1e-4, atol 1e-6).

Shapes: (320, 64) exact key tiles; (244, 64) tail tile; (153, 64) short tail; (720, 144) lens_t not a multiple of the
64-key tile, nine row blocks (three rounds of the four waves), K larger than the LDS; (427, 144) both.  Masks: one
row (27), the CTR_REC 2 x 2 block, 17 rows (one row in a second block: fifteen padding rows to weight out), every
row.  B = 1 and B = 3 with three different lists and counts in one launch.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS, C = 12, 768
SHAPES = [(320, 64), (244, 64), (153, 64), (720, 144), (427, 144)]


@pytest.fixture(scope="module")
def lib():
    from mmtrack_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def mask_rows(kind, lens_t):
    tf = int(round(lens_t ** 0.5))
    if kind == "one":
        return [27]
    if kind == "rec":
        i = {8: 3, 12: 5}[tf]
        return [r * tf + c for r in (i, i + 1) for c in (i, i + 1)]
    if kind == "r17":
        return [3 * i for i in range(17)]
    if kind == "all":
        return list(range(lens_t))
    raise KeyError(kind)


CASES = [("one",), ("rec",), ("r17",), ("all",), ("r17", "one", "all")]


def lists(kinds, lens_t):
    """Device rows [B][pitch] (unused entries -1: never read) and nrows [B]."""
    rows = -np.ones((len(kinds), lens_t), np.int32)
    nrows = np.zeros(len(kinds), np.int32)
    for b, k in enumerate(kinds):
        r = mask_rows(k, lens_t)
        rows[b, :len(r)] = r
        nrows[b] = len(r)
    return torch.from_numpy(rows).cuda(), torch.from_numpy(nrows).cuda()


def reference(q64, kinds, lens_t):
    """[B][heads][N - lens_t] from [B][N][3C] values, in the values' dtype."""
    B, N = q64.shape[:2]
    q, k, _ = q64.view(B, N, 3, HEADS, 64).permute(2, 0, 3, 1, 4)
    out = []
    for b, kind in enumerate(kinds):
        r = torch.tensor(mask_rows(kind, lens_t), device=q64.device)
        attn = ((q[b][:, r] @ k[b].transpose(-2, -1)) * 0.125).softmax(-1)   # [heads][rows][N]
        out.append(attn[:, :, lens_t:].mean(1))
    return torch.stack(out)


def make_qkv(N, B, lens_t):
    g = torch.Generator(device="cuda").manual_seed(11 * N + B + lens_t)
    return torch.randn(B, N, 3 * C, device="cuda", generator=g) * 1.5


def run_f16x3(lib, hi, lo, s, lens_t, rows, nrows):
    B, N = hi.shape[:2]
    prob = torch.full((B, HEADS, N - lens_t), float("nan"), device="cuda")
    rc = lib.mmt_op_ce_rows_f16x3(hi.data_ptr(), lo.data_ptr(), B, N, HEADS, lens_t, rows.data_ptr(), rows.shape[1],
                                  nrows.data_ptr(), prob.data_ptr(), s, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return prob


@pytest.mark.parametrize("kinds", CASES, ids=["-".join(k) for k in CASES])
@pytest.mark.parametrize("N,lens_t", SHAPES)
def test_ce_rows_f16x3_vs_fp64(lib, N, lens_t, kinds):
    qkv = make_qkv(N, len(kinds), lens_t)
    s = range_scale(qkv)
    hi, lo, q64 = split(qkv, s)
    rows, nrows = lists(kinds, lens_t)
    prob = run_f16x3(lib, hi, lo, s, lens_t, rows, nrows)
    ref = reference(q64, kinds, lens_t)
    err = float((prob.double() - ref).abs().max())
    print(f"f16x3 ce_rows N={N} lens_t={lens_t} {kinds}: max|dP| {err:.3e} (max P {float(ref.max()):.3e})")
    assert torch.isfinite(prob).all()
    assert err <= 1e-6
    if kinds == ("one",):
        # the same row through attention's single-row export
        out = torch.empty(1, N, C, device="cuda", dtype=torch.float16)
        out_lo = torch.empty_like(out)
        p1 = torch.empty_like(prob)
        rc = lib.mmt_op_attention_f16x3(hi.data_ptr(), lo.data_ptr(), out.data_ptr(), out_lo.data_ptr(), 1, N, HEADS, 27,
                                        lens_t, p1.data_ptr(), s, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        d = float((prob.double() - p1.double()).abs().max())
        print(f"  against attention's ce_query = 27 export: max|dP| {d:.3e}")
        assert d <= 1e-6


@pytest.mark.parametrize("kinds", CASES, ids=["-".join(k) for k in CASES])
@pytest.mark.parametrize("N,lens_t", SHAPES)
def test_ce_rows_bf16_vs_fp32(lib, N, lens_t, kinds):
    qkv = make_qkv(N, len(kinds), lens_t).to(torch.bfloat16)
    rows, nrows = lists(kinds, lens_t)
    B = len(kinds)
    prob = torch.full((B, HEADS, N - lens_t), float("nan"), device="cuda")
    rc = lib.mmt_op_ce_rows(qkv.data_ptr(), B, N, HEADS, lens_t, rows.data_ptr(), rows.shape[1], nrows.data_ptr(),
                            prob.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    ref = reference(qkv.float(), kinds, lens_t)
    print(f"bf16 ce_rows N={N} lens_t={lens_t} {kinds}: max|dP| {float((prob - ref).abs().max()):.3e}")
    torch.testing.assert_close(prob, ref, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("N,lens_t", [(427, 144), (244, 64)])
def test_ce_rows_same_bits_again_and_anywhere_in_the_batch(lib, N, lens_t):
    """No atomics and a fixed summation order: a rerun gives the same bits, and a sequence's result does not depend
    on the batch size or on its place in the batch."""
    kinds = ("r17", "one", "all")
    qkv = make_qkv(N, 3, lens_t)
    s = range_scale(qkv)
    hi, lo, _ = split(qkv, s)
    rows, nrows = lists(kinds, lens_t)
    a = run_f16x3(lib, hi, lo, s, lens_t, rows, nrows)
    b = run_f16x3(lib, hi, lo, s, lens_t, rows, nrows)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for i in range(3):
        one = run_f16x3(lib, hi[i:i + 1].contiguous(), lo[i:i + 1].contiguous(), s, lens_t, rows[i:i + 1].contiguous(),
                        nrows[i:i + 1].contiguous())
        assert torch.equal(one.view(torch.int32)[0], a.view(torch.int32)[i])


def test_ce_rows_bad_arguments(lib):
    """nrows = 0, a row >= lens_t and lens_t >= N are MMT_E_ARG (-1) before any launch: the output stays untouched."""
    N, lens_t = 153, 64
    qkv = make_qkv(N, 1, lens_t).to(torch.bfloat16)
    s = 1024.0
    hi = qkv.to(torch.float16)
    prob = torch.full((1, HEADS, N - lens_t), -7.0, device="cuda")

    def both(rows, nrows, lt=lens_t, n=N):
        rc1 = lib.mmt_op_ce_rows(qkv.data_ptr(), 1, n, HEADS, lt, rows.data_ptr(), rows.shape[1], nrows.data_ptr(),
                                 prob.data_ptr(), _stream())
        rc2 = lib.mmt_op_ce_rows_f16x3(hi.data_ptr(), hi.data_ptr(), 1, n, HEADS, lt, rows.data_ptr(), rows.shape[1],
                                       nrows.data_ptr(), prob.data_ptr(), s, _stream())
        torch.cuda.synchronize()
        return rc1, rc2

    rows, nrows = lists(("rec",), lens_t)
    assert both(rows, torch.zeros_like(nrows)) == (-1, -1)
    bad = rows.clone()
    bad[0, 3] = lens_t
    assert both(bad, nrows) == (-1, -1)
    assert both(rows, nrows, lt=N) == (-1, -1)
    assert both(rows, nrows, lt=N + 5) == (-1, -1)
    assert bool((prob == -7.0).all())
    assert both(rows, nrows) == (0, 0)
    assert bool((prob != -7.0).all())
