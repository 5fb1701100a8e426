"""Operator-level tests of the token kernels (csrc/tokens.hip) against float64 references (GPU only).

Bitwise tests pin the claims the kernels' comments make: the CE order (key descending, ties to the lower index), the
fused CE + LN2 launch against the two launches it replaces, the split-K RowReduce against the reduce arithmetic, one
ln_row in every kernel that inlines it, the f16x3 halves, the block partition (1, 2, 4 slots per wave) and the fovea
statistics handed from one layer's LN1 to the next layer's prompt kernel.

Value tests compare with float64 torch on the same fp32 inputs.  LayerNorm outputs: the bar of test_layernorm
(rtol = atol = 1e-4, bf16 1e-2).  768-long dot products (a8, layer-0 c8): (768 + 16) 2^-24 sum |a_i b_i| plus the
LayerNorm bar propagated through sum |w|.  Outputs behind the fovea softmax and the PromptFold (deep c8, X, the
statistics) have no derivable bar: the same unfolded formula is evaluated in fp32 torch on the CPU and the kernel may
be 8 times as far from float64 as that, floored at the dot-product bar of the output.

Worst observed kernel error / fp32-reference error (MI355X; every case, the three smooth settings): deep c8 0.52
(the fold is closer to float64 than the unfolded fp32 chain), mode-1 X 1.15, mode-2 X 1.05, fovea statistics 1.46
(mode 1) and 1.95 (mode 2) -- all far inside the factor 8.  The 768-long dot products (layer-0 a8 / c8, deep a8) sit
at 1.5e-4 of their derived worst-case bar (errors below 1.1e-6).  LayerNorm on rows x * 0.01 + 50 misses the 1e-4 bar
as any fp32 LayerNorm does: kernel 1.12e-3, torch's fp32 layer_norm 9.2e-4 on the same rows (ratio 1.21, bar 4).

Each bitwise test was seen to fail against a library with one memory-safe arithmetic change in the code it pins: ties
to the higher index in before(), a division for the mean in the fused CE kernel's LayerNorm, the split-K slabs summed
in reverse, a scaled smooth in the third and fourth slot of a wave, a slot dropped from the fovea sum's LDS branch.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 768
EPS = 1e-6
U = 2.0 ** -24
GEOS = [(4, 9), (64, 256), (64, 257), (144, 576), (256, 768)]
# (Lz, Lx, B): every geometry, B in {1, 2, 3, 8} (one slot per wave below 8 sequences, two from 8)
CASES = [(4, 9, 3), (4, 9, 8), (64, 256, 1), (64, 256, 8), (64, 257, 2), (144, 576, 2), (256, 768, 1)]


@pytest.fixture(scope="module")
def lib():
    from mmtrack_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def nan_rows(rows, cols, dtype=torch.float32):
    """rows + 1 NaN rows: the outputs of a launch and one guard row after them."""
    return torch.full((rows + 1, cols), float("nan"), device="cuda", dtype=dtype)


def check_guard(t, rows, what):
    assert torch.isnan(t[rows].float()).all(), f"{what}: a store past the last row"
    assert not torch.isnan(t[:rows].float()).any(), f"{what}: a row left unwritten"


def reduce_arg(ws, inv, bias):
    """mmt_row_reduce over ws [ks][rows][768]."""
    from mmtrack_amd import _lib
    if ws is None:
        return None
    return ctypes.byref(_lib.MmtRowReduce(ws.data_ptr(), ws.shape[0], ws[0].numel(), inv, bias.data_ptr()))


def reduced(x, ws, inv, bias):
    """x + ((p0 + p1) + ...) * inv + bias in fp32, slabs in order (inv a power of two: one rounding, as the fmaf)."""
    acc = ws[0].clone()
    for k in range(1, ws.shape[0]):
        acc = acc + ws[k]
    return x + (acc * inv + bias)


def split_host(y, s):
    """tests/test_gpu_f16x3.py::split on the host: fp32 multiply, RNE to half, fp32 subtract, RNE."""
    v = y.detach().float().cpu() * s
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi, lo


def ln_ex(lib, x, w, b, rows, out=None, out_lo=None, scale=1.0, of=None, rps=None, gather=None, in_rps=0, xcopy=None,
          rr=None, expect=0):
    rc = lib.mmt_op_layernorm_ex(P(x), P(w), P(b), P(out), P(out_lo), scale, P(of), rows, rps or rows, P(gather),
                                 in_rps or (rps or rows), P(xcopy), rr, _stream())
    assert rc == expect, rc
    torch.cuda.synchronize()


def affine(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(C, device="cuda", generator=g) * 0.3 + 1, torch.randn(C, device="cuda", generator=g) * 0.2)


# --------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows", [1, 1024, 1025, 1027])
def test_layernorm_ex_values_and_split(lib, rows):
    """f32 / bf16 / f16x3 outputs at both rows-per-block sides (1 row per block up to 1 024 rows, 4 above, a partial
    last block of four at 1 025 and 1 027); the halves are bit for bit the split of the launch's own f32 rows."""
    g = torch.Generator(device="cuda").manual_seed(rows)
    x = torch.randn(rows, C, device="cuda", generator=g) * 3 + 1
    w, b = affine(rows + 1)
    ref = F.layer_norm(x.double().cpu(), (C,), w.double().cpu(), b.double().cpu(), EPS)
    of, ob = nan_rows(rows, C), nan_rows(rows, C, torch.bfloat16)
    ln_ex(lib, x, w, b, rows, out=ob, of=of)
    check_guard(of, rows, "f32")
    check_guard(ob, rows, "bf16")
    torch.testing.assert_close(of[:rows].double().cpu(), ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ob[:rows].double().cpu(), ref, rtol=1e-2, atol=1e-2)
    of2, hi, lo = nan_rows(rows, C), nan_rows(rows, C, torch.float16), nan_rows(rows, C, torch.float16)
    ln_ex(lib, x, w, b, rows, out=hi, out_lo=lo, scale=2048.0, of=of2)
    for t in (of2, hi, lo):
        check_guard(t, rows, "split")
    assert torch.equal(of2[:rows], of[:rows])
    eh, el = split_host(of2[:rows], 2048.0)
    assert torch.equal(hi[:rows].cpu(), eh) and torch.equal(lo[:rows].cpu(), el)


def test_layernorm_ex_edge_rows(lib):
    """Rows with mean >> std, an all-zero row (the result is the LN bias exactly) and a constant row."""
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(8, C, device="cuda", generator=g)
    x[:4] = x[:4] * 0.01 + 50
    x[4] = 0
    x[5] = 3.0
    w, b = affine(6)
    ref = F.layer_norm(x.double().cpu(), (C,), w.double().cpu(), b.double().cpu(), EPS)
    of = nan_rows(8, C)
    ln_ex(lib, x, w, b, 8, of=of)
    check_guard(of, 8, "f32")
    got = of[:8].double().cpu()
    assert torch.equal(of[4], b)
    torch.testing.assert_close(got[4:], ref[4:], rtol=1e-4, atol=1e-4)
    # offset-mean rows: the project's bar, or where fp32 cannot hold it, 4 x the error of torch's own fp32 LayerNorm
    t32 = F.layer_norm(x.cpu(), (C,), w.cpu(), b.cpu(), EPS).double()
    e_k, e_t = (got[:4] - ref[:4]).abs().max().item(), (t32[:4] - ref[:4]).abs().max().item()
    print(f"layernorm, rows x * 0.01 + 50: kernel max |err| {e_k:.3e}, torch fp32 {e_t:.3e}, ratio {e_k / e_t:.2f}")
    in_bar = ((got[:4] - ref[:4]).abs() <= 1e-4 + 1e-4 * ref[:4].abs()).all().item()
    assert in_bar or e_k <= 4 * e_t


def test_layernorm_ex_rejects(lib):
    x = torch.zeros(4, C, device="cuda")
    w, b = affine(1)
    of = nan_rows(4, C)
    ws = torch.zeros(9, 4, C, device="cuda")
    ln_ex(lib, x, w, b, 4, of=of, rr=reduce_arg(ws, 1.0, b), expect=-1)       # ks = 9
    ln_ex(lib, x, w, b, 0, of=of, expect=-1)
    ln_ex(lib, x, w, b, 4, expect=-1)                                         # no output
    bad = torch.tensor([0, 1, 2, 4], device="cuda", dtype=torch.int32)
    ln_ex(lib, x, w, b, 4, of=of, gather=bad, in_rps=4, expect=-1)            # gather out of range
    assert torch.isnan(of).all()                                              # nothing was launched
    assert lib.mmt_tokens_force_config(3, -1) == -1 and lib.mmt_tokens_force_config(-1, 2) == -1


# --------------------------------------------------------------------------------------------- candidate elimination
def ce_inputs(B, Ls, heads, pattern, seed):
    g = torch.Generator().manual_seed(seed)
    prob = torch.rand(B, heads, Ls, generator=g) * 0.01
    if pattern == "ties":     # scattered groups of bit-identical columns
        ngroups = max(2, Ls // 7)   # groups of 7 or 8 columns
        col = torch.stack([torch.randperm(Ls, generator=g) % ngroups for _ in range(B)])
        prob = torch.gather(prob, 2, col[:, None, :].expand(B, heads, Ls))
    elif pattern == "equal":
        prob = prob[:, :, :1].expand(B, heads, Ls).contiguous()
    return prob.contiguous()


def ce_expected(prob, gidx_in, Lz, Lx, keep, removed_off, fill):
    """The index arrays from keys formed with the kernel's arithmetic (heads summed in order, then / heads, fp32),
    ordered by (-key, index)."""
    B, heads, Ls = prob.shape
    key = torch.zeros(B, Ls)
    for h in range(heads):
        key = key + prob[:, h]
    key = torch.from_numpy(key.numpy() / np.float32(heads))
    order = torch.sort(-key, dim=1, stable=True).indices
    slots = torch.gather(gidx_in.long(), 1, order)
    gidx_out = slots[:, :keep]
    gather = torch.cat([torch.arange(Lz).expand(B, Lz), Lz + order[:, :keep]], 1)
    slot2pos = torch.full((B, Lx), fill, dtype=torch.long)
    slot2pos.scatter_(1, slots[:, :keep], (Lz + torch.arange(keep)).expand(B, keep))
    slot2pos.scatter_(1, slots[:, keep:], torch.full((B, Ls - keep), -1, dtype=torch.long))
    removed = torch.full((B, Lx), fill, dtype=torch.long)
    removed[:, removed_off:removed_off + Ls - keep] = slots[:, keep:]
    return key, order, gidx_out.int(), gather.int(), slot2pos.int(), removed.int()


def run_ce(lib, prob, gidx_in, Lz, Lx, keep, removed_off, fused, x, w, b, in_rps, out=None, out_lo=None, scale=1.0,
           xcopy=None, rr=None, fill=-7, expect=0):
    from mmtrack_amd import _lib
    B, heads, Ls = prob.shape
    dev = dict(gidx_out=torch.full((B * keep + 1,), fill, device="cuda", dtype=torch.int32),
               gather=torch.full((B * (Lz + keep) + 1,), fill, device="cuda", dtype=torch.int32),
               slot2pos=torch.full((B * Lx + 1,), fill, device="cuda", dtype=torch.int32),
               removed=torch.full((B * Lx + 1,), fill, device="cuda", dtype=torch.int32))
    a = _lib.MmtCeArgs(B, Lz, Ls, keep, heads, Lx, prob.data_ptr(), gidx_in.data_ptr(), dev["gidx_out"].data_ptr(),
                       dev["gather"].data_ptr(), dev["slot2pos"].data_ptr(), dev["removed"].data_ptr(), removed_off)
    rc = lib.mmt_op_ce_select(ctypes.byref(a), fused, P(x), P(w), P(b), P(out), P(out_lo), scale, in_rps, P(xcopy), rr,
                              _stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    for k, v in dev.items():
        assert v[-1].item() == fill, f"{k}: a store past the end"
    return {k: v[:-1].cpu() for k, v in dev.items()}


CE_CASES = [  # Ls, heads, keep, pattern, (Lx, removed_off) of a second stage or None
    (9, 12, 5, "rand", None), (9, 1, 1, "ties", None), (9, 20, 9, "equal", None),
    (256, 12, 180, "rand", None), (256, 16, 131, "ties", None), (256, 20, 1, "equal", None),
    (257, 20, 104, "ties", None), (257, 12, 257, "rand", None),
    (576, 12, 403, "rand", None), (576, 16, 1, "ties", None), (576, 1, 300, "equal", None),
    (1024, 20, 717, "ties", None), (1024, 1, 1024, "equal", None), (1024, 12, 512, "rand", None),
    (179, 12, 125, "ties", (256, 77)), (403, 16, 282, "rand", (576, 173)),
]


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("Ls,heads,keep,pattern,stage2", CE_CASES)
def test_ce_select_order(lib, Ls, heads, keep, pattern, stage2, fused):
    """gidx_out, gather, slot2pos and the removed segment, in order: key descending, exact ties to the lower index
    (ties straddle the keep boundary), keep == Ls and keep == 1, 1 / 12 / 16 / 20 heads (the tail loop beyond 16),
    a second stage with a non-identity gidx_in, removed_off > 0 and Ls < Lx."""
    B = 2 if fused else 3
    Lz = 4 if Ls == 9 else 64
    Lx, removed_off = stage2 or (Ls, 0)
    prob = ce_inputs(B, Ls, heads, pattern, 7 * Ls + heads + keep)
    g = torch.Generator().manual_seed(Ls)
    if stage2:   # the Ls survivors of a first stage, in some order
        gidx_in = torch.stack([torch.randperm(Lx, generator=g)[:Ls] for _ in range(B)]).int()
    else:
        gidx_in = torch.arange(Ls).expand(B, Ls).contiguous().int()
    key, order, *want = ce_expected(prob, gidx_in, Lz, Lx, keep, removed_off, -7)
    if pattern != "rand" and keep < Ls:
        kk = torch.gather(key, 1, order)
        assert (kk[:, keep - 1] == kk[:, keep]).all(), "the case should put an exact tie on the keep boundary"
    x = torch.randn(B, Lz + Ls, C, generator=g).cuda()
    w, b = affine(3)
    out = nan_rows(B * (Lz + keep), C, torch.bfloat16)
    got = run_ce(lib, prob.cuda(), gidx_in.cuda(), Lz, Lx, keep, removed_off, fused, x, w, b, Lz + Ls, out=out)
    check_guard(out, B * (Lz + keep), "LN2")
    for name, wv in zip(("gidx_out", "gather", "slot2pos", "removed"), want):
        assert torch.equal(got[name], wv.reshape(-1)), name


def test_ce_select_rejects(lib):
    """Ls = 1025 (the keys' LDS array holds 1 024), keep > Ls, keep < 1, heads < 1: MMT_E_ARG, nothing launched."""
    from mmtrack_amd import _lib
    Lz = 4
    w, b = affine(3)
    for Ls, keep, heads in [(1025, 700, 12), (9, 10, 12), (9, 0, 12), (9, 5, 0)]:
        prob = torch.rand(1, max(heads, 1), Ls, device="cuda")
        gidx = torch.arange(Ls, device="cuda", dtype=torch.int32)[None].contiguous()
        x = torch.zeros(1, Lz + Ls, C, device="cuda")
        out = nan_rows(Lz + max(keep, 1), C, torch.bfloat16)
        for fused in (0, 1):
            dummy = torch.full((Ls + Lz + 8,), -7, device="cuda", dtype=torch.int32)
            a = _lib.MmtCeArgs(1, Lz, Ls, keep, heads, Ls, prob.data_ptr(), gidx.data_ptr(), dummy.data_ptr(),
                               dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), 0)
            rc = lib.mmt_op_ce_select(ctypes.byref(a), fused, P(x), P(w), P(b), P(out), None, 1.0, Lz + Ls, None, None,
                                      _stream())
            assert rc == -1
            torch.cuda.synchronize()
            assert (dummy == -7).all() and torch.isnan(out.float()).all()


def test_ce_fused_declines_three_sequences(lib):
    """fused = 1 where the one-launch kernel does not take the batch (more than two sequences): MMT_E_STATE and
    nothing launched -- no quiet fall-back to the two launches."""
    B, Lz, Ls, keep = 3, 4, 9, 5
    prob = ce_inputs(B, Ls, 12, "rand", 1).cuda()
    gidx = torch.arange(Ls).expand(B, Ls).contiguous().int().cuda()
    x = torch.zeros(B, Lz + Ls, C, device="cuda")
    w, b = affine(3)
    out = nan_rows(B * (Lz + keep), C, torch.bfloat16)
    got = run_ce(lib, prob, gidx, Lz, Ls, keep, 0, 1, x, w, b, Lz + Ls, out=out, expect=-2)
    assert all((v == -7).all() for v in got.values()) and torch.isnan(out.float()).all()


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ks", [0, 3])
@pytest.mark.parametrize("Lz,Ls,keep", [(4, 9, 5), (64, 256, 180), (144, 30, 9)])
@pytest.mark.parametrize("split", [False, True])
def test_ce_fused_matches_unfused(lib, Lz, Ls, keep, B, ks, split):
    """ce_ln_kernel forms "the same sums in the same order" as ce_select + ln_kernel: identical index arrays,
    bit-identical LN2 rows (bf16, or hi / lo), xcopy and written-back X, with and without a RowReduce.  Compact
    lengths 9, 244, 153."""
    g = torch.Generator().manual_seed(Lz + Ls + B)
    prob = ce_inputs(B, Ls, 12, "ties", Ls + B).cuda()
    gidx_in = torch.stack([torch.randperm(Ls, generator=g) for _ in range(B)]).int().cuda()
    x0 = torch.randn(B, Lz + Ls, C, generator=g).cuda()
    w, b = affine(4)
    ws = (torch.randn(ks, B * (Lz + Ls), C, generator=g) * 0.3).cuda() if ks else None
    bias = torch.randn(C, generator=g).cuda()
    n = B * (Lz + keep)
    res = []
    for fused in (0, 1):
        x = x0.clone()
        dt = torch.float16 if split else torch.bfloat16
        out, lo = nan_rows(n, C, dt), nan_rows(n, C, dt) if split else None
        xcopy = None if split else nan_rows(n, C)   # split case: the update is written back to X instead
        got = run_ce(lib, prob, gidx_in, Lz, Ls, keep, 0, fused, x, w, b, Lz + Ls, out=out, out_lo=lo,
                     scale=512.0 if split else 1.0, xcopy=xcopy, rr=reduce_arg(ws, 0.25, bias))
        check_guard(out, n, "LN2")
        res.append((got, out, lo, xcopy, x))
    (g0, o0, l0, c0, xa), (g1, o1, l1, c1, xb) = res
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert torch.equal(o0[:n], o1[:n]) and torch.equal(xa, xb)
    if split:
        assert torch.equal(l0[:n], l1[:n])
        if ks:   # the gathered source rows were updated in place, bit for bit the reduce arithmetic; the rest untouched
            src = (torch.arange(B)[:, None] * (Lz + Ls) + g0["gather"].reshape(B, -1).long()).reshape(-1).cuda()
            want = x0.reshape(-1, C).clone()
            want[src] = reduced(x0.reshape(-1, C), ws, 0.25, bias)[src]
            assert torch.equal(xb.reshape(-1, C), want)
    else:
        check_guard(c0, n, "xcopy")
        assert torch.equal(c0[:n], c1[:n]) and torch.equal(xa, x0)


# --------------------------------------------------------------------------------------------- one ln_row everywhere
def test_ln_row_one_arithmetic(lib):
    """ln_row "rounds identically in every kernel that inlines it": the same X rows through layernorm_ex with 1 and
    4 rows per block, the gathered launch, the fused CE launch and the live rows of final_norm_recover."""
    B, Lz, Ls, keep = 2, 4, 9, 5
    Na, Ln = Lz + Ls, Lz + keep
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(B, Na, C, generator=g) * 2 + 0.5).cuda()
    w, b = affine(8)
    s = 1024.0
    base = {}
    try:
        for rpb in (1, 4):
            assert lib.mmt_tokens_force_config(-1, rpb) == 0
            of, hi, lo = nan_rows(B * Na, C), nan_rows(B * Na, C, torch.float16), nan_rows(B * Na, C, torch.float16)
            ln_ex(lib, x, w, b, B * Na, out=hi, out_lo=lo, scale=s, of=of)
            # final norm over the uneliminated sequence: every slot live, slot2pos the identity
            s2p = (Lz + torch.arange(Ls)).expand(B, Ls).contiguous().int().cuda()
            fh, fl, ff = (nan_rows(B * Ls, C, torch.float16), nan_rows(B * Ls, C, torch.float16), nan_rows(B * Na, C))
            assert lib.mmt_op_final_norm_recover(P(x), Na, P(s2p), P(w), P(b), B, Lz, Ls, P(fh), P(fl), s, P(ff), None,
                                                 _stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(ff[:B * Na], of[:B * Na])
            sel = (torch.arange(B)[:, None] * Na + Lz + torch.arange(Ls)).reshape(-1).cuda()
            assert torch.equal(fh[:B * Ls], hi[sel]) and torch.equal(fl[:B * Ls], lo[sel])
            base[rpb] = (of[:B * Na], hi[:B * Na], lo[:B * Na])
        assert all(torch.equal(p, q) for p, q in zip(base[1], base[4]))
    finally:
        lib.mmt_tokens_force_config(-1, -1)
    of, hi, lo = base[1]
    # the gathered launch
    gat = torch.stack([torch.cat([torch.arange(Lz), Lz + torch.randperm(Ls, generator=g)[:keep]]) for _ in range(B)])
    src = (torch.arange(B)[:, None] * Na + gat).reshape(-1).cuda()
    gh, gl, gf = nan_rows(B * Ln, C, torch.float16), nan_rows(B * Ln, C, torch.float16), nan_rows(B * Ln, C)
    ln_ex(lib, x, w, b, B * Ln, out=gh, out_lo=gl, scale=s, of=gf, rps=Ln, gather=gat.int().cuda(), in_rps=Na)
    assert torch.equal(gf[:B * Ln], of[src]) and torch.equal(gh[:B * Ln], hi[src]) and torch.equal(gl[:B * Ln], lo[src])
    # the fused CE launch
    prob = ce_inputs(B, Ls, 12, "rand", 5).cuda()
    gidx = torch.arange(Ls).expand(B, Ls).contiguous().int().cuda()
    ch, cl = nan_rows(B * Ln, C, torch.float16), nan_rows(B * Ln, C, torch.float16)
    got = run_ce(lib, prob, gidx, Lz, Ls, keep, 0, 1, x, w, b, Na, out=ch, out_lo=cl, scale=s)
    src = (torch.arange(B)[:, None] * Na + got["gather"].reshape(B, Ln).long()).reshape(-1).cuda()
    assert torch.equal(ch[:B * Ln], hi[src]) and torch.equal(cl[:B * Ln], lo[src])


# --------------------------------------------------------------------------------------------- RowReduce
@pytest.mark.parametrize("ks", [1, 2, 3, 8])
@pytest.mark.parametrize("rows", [5, 1027])
def test_row_reduce_layernorm(lib, ks, rows):
    """The consumer forms "the bits of the splitk_reduce launch this replaces": X written back (or xcopy) equals
    x + ((p0 + p1) + ...) * inv + bias in fp32 bit for bit, and the LN is that of the reduced row."""
    g = torch.Generator(device="cuda").manual_seed(ks * 10 + rows)
    x0 = torch.randn(rows, C, device="cuda", generator=g)
    ws = torch.randn(ks, rows, C, device="cuda", generator=g) * 0.5
    bias = torch.randn(C, device="cuda", generator=g)
    w, b = affine(2)
    want = reduced(x0, ws, 0.125, bias)
    of_ref = nan_rows(rows, C)
    ln_ex(lib, want, w, b, rows, of=of_ref)
    x, of = torch.cat([x0, nan_rows(0, C)]), nan_rows(rows, C)
    ln_ex(lib, x, w, b, rows, of=of, rr=reduce_arg(ws, 0.125, bias))
    assert torch.equal(x[:rows], want) and torch.isnan(x[rows]).all() and torch.equal(of[:rows], of_ref[:rows])
    x, of, xc = x0.clone(), nan_rows(rows, C), nan_rows(rows, C)
    ln_ex(lib, x, w, b, rows, of=of, xcopy=xc, rr=reduce_arg(ws, 0.125, bias))
    check_guard(xc, rows, "xcopy")
    assert torch.equal(xc[:rows], want) and torch.equal(x, x0) and torch.equal(of[:rows], of_ref[:rows])


@pytest.mark.parametrize("ks", [1, 2, 3, 8])
def test_row_reduce_final_norm(lib, ks):
    """final_norm_recover applies the update without writing X: its f32 rows are layernorm_ex of the reduced X; pruned
    slots are exact zeros in every output; template rows reach only the f32 output."""
    B, Lz, Lx, keep = 3, 4, 9, 6
    Na = Lz + keep
    g = torch.Generator().manual_seed(ks)
    x0 = torch.randn(B * Na, C, generator=g).cuda()
    ws = (torch.randn(ks, B * Na, C, generator=g) * 0.5).cuda()
    bias = torch.randn(C, generator=g).cuda()
    w, b = affine(9)
    s2p = torch.full((B, Lx), -1, dtype=torch.int32)
    for bb in range(B):
        s2p[bb, torch.randperm(Lx, generator=g)[:keep]] = (Lz + torch.arange(keep)).int()
    want_x = reduced(x0, ws, 0.5, bias)
    ln_ref = nan_rows(B * Na, C)
    ln_ex(lib, want_x, w, b, B * Na, of=ln_ref)
    x = x0.clone()
    fh, fl, ff = nan_rows(B * Lx, C, torch.float16), nan_rows(B * Lx, C, torch.float16), nan_rows(B * (Lz + Lx), C)
    assert lib.mmt_op_final_norm_recover(P(x), Na, P(s2p.cuda()), P(w), P(b), B, Lz, Lx, P(fh), P(fl), 256.0, P(ff),
                                         reduce_arg(ws, 0.5, bias), _stream()) == 0
    torch.cuda.synchronize()
    for t, n in ((fh, B * Lx), (fl, B * Lx), (ff, B * (Lz + Lx))):
        check_guard(t, n, "final norm")
    assert torch.equal(x, x0)
    ff3, ln3 = ff[:B * (Lz + Lx)].reshape(B, Lz + Lx, C), ln_ref[:B * Na].reshape(B, Na, C)
    assert torch.equal(ff3[:, :Lz], ln3[:, :Lz])
    live = s2p >= 0
    for bb in range(B):
        assert torch.equal(ff3[bb, Lz:][live[bb]], ln3[bb][s2p[bb][live[bb]].long()])
        assert (ff3[bb, Lz:][~live[bb]] == 0).all()
    eh, el = split_host(ff3[:, Lz:].reshape(-1, C), 256.0)
    assert torch.equal(fh[:B * Lx].cpu(), eh) and torch.equal(fl[:B * Lx].cpu(), el)
    dead = (~live).reshape(-1)
    assert (fh[:B * Lx].cpu()[dead].view(torch.int16) == 0).all() and (fl[:B * Lx].cpu()[dead].view(torch.int16) == 0).all()
    # bf16 features, and a RowReduce of 9 slabs
    fb = nan_rows(B * Lx, C, torch.bfloat16)
    assert lib.mmt_op_final_norm_recover(P(x), Na, P(s2p.cuda()), P(w), P(b), B, Lz, Lx, P(fb), None, 1.0, None,
                                         reduce_arg(ws, 0.5, bias), _stream()) == 0
    torch.cuda.synchronize()
    check_guard(fb, B * Lx, "bf16 features")
    assert torch.equal(fb[:B * Lx], ff3[:, Lz:].reshape(-1, C).bfloat16())
    ws9 = torch.zeros(9, 1, C, device="cuda")
    fb2 = nan_rows(B * Lx, C, torch.bfloat16)
    assert lib.mmt_op_final_norm_recover(P(x), Na, P(s2p.cuda()), P(w), P(b), B, Lz, Lx, P(fb2), None, 1.0, None,
                                         reduce_arg(ws9, 0.5, bias), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(fb2.float()).all()


# --------------------------------------------------------------------------------------------- the prompt pipeline
@pytest.fixture(scope="module")
def W(lib):
    """Prompt blocks 0 and 1, their norms and block 0 / 1's norm1 of the synthetic ViPT-deep state dict, and layer
    1's folded constants from mmt_prompt_fold."""
    from mmtrack_amd import synth
    sd = synth.make_state_dict(0, kind="vipt", prompt_type="vipt_deep")
    w = {}
    for i in (0, 1):
        p = f"backbone.prompt_blocks.{i}."
        w[i] = dict(w00=sd[p + "conv0_0.weight"].reshape(8, C), b00=sd[p + "conv0_0.bias"],
                    w01=sd[p + "conv0_1.weight"].reshape(8, C), b01=sd[p + "conv0_1.bias"],
                    V=sd[p + "conv1x1.weight"].reshape(C, 8).contiguous(), v0=sd[p + "conv1x1.bias"],
                    smooth=float(sd[p + "fovea.smooth"][0]), ng=sd[f"backbone.prompt_norms.{i}.weight"],
                    nb=sd[f"backbone.prompt_norms.{i}.bias"], n1w=sd[f"backbone.blocks.{i}.norm1.weight"],
                    n1b=sd[f"backbone.blocks.{i}.norm1.bias"])
        w[i]["w1t"] = w[i]["V"].t().contiguous()
    ins = [w[1]["w00"], w[1]["b00"], w[0]["ng"], w[0]["nb"], w[1]["w01"], w[1]["b01"], w[1]["ng"], w[1]["nb"],
           w[0]["V"], w[0]["v0"]]
    ins = [np.ascontiguousarray(t.numpy().reshape(-1)) for t in ins]
    outs = [np.zeros(8 * C, np.float32), np.zeros(8, np.float32), np.zeros(160, np.float32)]
    assert lib.mmt_prompt_fold(*[a.ctypes.data_as(ctypes.c_void_p) for a in ins + outs]) == 0
    w[1]["w00f"], w[1]["b00f"], w[1]["fold"] = (torch.from_numpy(o) for o in outs)
    w[1]["w00f"] = w[1]["w00f"].reshape(8, C)
    w["dev"] = {i: {k: v.cuda() for k, v in w[i].items() if torch.is_tensor(v)} for i in (0, 1)}
    return w


def run_pipeline(lib, W, Lz, Lx, B, big_smooth=False, use_fstat=True, ks=0):
    """Layer-0 prompt_reduce -> prompt_expand_ln mode 1 -> (a shuffled, shortened compact sequence) -> deep
    prompt_reduce -> prompt_expand_ln mode 2, every output NaN-filled with a guard row.  Returns CPU tensors."""
    from mmtrack_amd import _lib
    L = Lz + Lx
    d0, d1 = W["dev"][0], W["dev"][1]
    # fovea.smooth: the state dict's (8 .. 12), a larger one (a peaked softmax: the max subtraction matters) or a
    # small one (a flat softmax: every slot of the part carries the same weight in the sum)
    sm0 = {False: W[0]["smooth"], True: 16.0, "flat": 0.0625}[big_smooth]
    sm1 = {False: W[1]["smooth"], True: 12.5, "flat": 0.03125}[big_smooth]
    g = torch.Generator().manual_seed(1000 * Lz + 10 * Lx + B)
    tok_rgb, tok_aux = (torch.randn(B * L, C, generator=g) * 0.5).cuda(), (torch.randn(B * L, C, generator=g) * 0.5 + 0.1).cuda()
    pos = (torch.randn(L, C, generator=g) * 0.5).cuda()
    r = dict(Lz=Lz, Lx=Lx, B=B, sm0=sm0, sm1=sm1, tok_rgb=tok_rgb.cpu(), tok_aux=tok_aux.cpu(), pos=pos.cpu())
    # layer 0
    a8_0, c8_0 = nan_rows(B * L, 8), nan_rows(B * L, 8)
    a = _lib.MmtPromptArgs(layer=0, B=B, Lz=Lz, Lx=Lx, srcA=P(tok_rgb), srcA_rows=L, srcB=P(tok_aux), lnA_w=P(d0["ng"]),
                           lnA_b=P(d0["nb"]), lnB_w=P(d0["ng"]), lnB_b=P(d0["nb"]), w00=P(d0["w00"]), b00=P(d0["b00"]),
                           w01=P(d0["w01"]), b01=P(d0["b01"]), a8=P(a8_0), c8=P(c8_0))
    assert lib.mmt_op_prompt_reduce(ctypes.byref(a), None, _stream()) == 0
    X0, h0, l0, fs0 = nan_rows(B * L, C), nan_rows(B * L, C, torch.float16), nan_rows(B * L, C, torch.float16), nan_rows(B, 32)
    la = _lib.MmtLnPromptArgs(mode=1, rows=B * L, rows_per_seq=L, Lz=Lz, Lx=Lx, X=P(X0), a8=P(a8_0), c8=P(c8_0),
                              smooth=sm0, fstat=P(fs0), w1=P(d0["w1t"]), b1=P(d0["v0"]), tok_rgb=P(tok_rgb), pos=P(pos),
                              w=P(d0["n1w"]), b=P(d0["n1b"]), out=P(h0), out_lo=P(l0), out_scale=256.0)
    assert lib.mmt_op_prompt_expand_ln(ctypes.byref(la), _stream()) == 0
    torch.cuda.synchronize()
    # the compact sequence after an elimination: keep of the Lx slots, in some order
    keep = max(1, Lx * 7 // 10)
    Na = Lz + keep
    gidx = torch.stack([torch.randperm(Lx, generator=g)[:keep] for _ in range(B)]).int()
    s2p = torch.full((B, Lx), -1, dtype=torch.int32)
    s2p.scatter_(1, gidx.long(), (Lz + torch.arange(keep)).expand(B, keep).int())
    X1_in = torch.cat([torch.randn(B * Na, C, generator=g).cuda(), nan_rows(0, C)])
    ws = (torch.randn(ks, B * Na, C, generator=g) * 0.5).cuda() if ks else None
    bias = torch.randn(C, generator=g).cuda()
    X1 = X1_in.clone()
    gidx_d, s2p_d = gidx.cuda(), s2p.cuda()
    a8_1, c8_1 = nan_rows(B * L, 8), nan_rows(B * L, 8)
    a = _lib.MmtPromptArgs(layer=1, B=B, Lz=Lz, Lx=Lx, srcA=P(X1), srcA_rows=Na, slot2pos=P(s2p_d), w00=P(d1["w00f"]),
                           b00=P(d1["b00f"]), fold=P(d1["fold"]), a8=P(a8_1), c8=P(c8_1), a8p=P(a8_0), c8p=P(c8_0),
                           smooth_p=sm0, fstat_p=P(fs0) if use_fstat else None)
    assert lib.mmt_op_prompt_reduce(ctypes.byref(a), reduce_arg(ws, 0.25, bias), _stream()) == 0
    torch.cuda.synchronize()
    X1_mid = X1.clone()
    h1, fs1 = nan_rows(B * Na, C, torch.bfloat16), nan_rows(B, 32)
    la = _lib.MmtLnPromptArgs(mode=2, rows=B * Na, rows_per_seq=Na, Lz=Lz, Lx=Lx, X=P(X1), a8=P(a8_1), c8=P(c8_1),
                              smooth=sm1, fstat=P(fs1), w1=P(d1["w1t"]), b1=P(d1["v0"]), gidx=P(gidx_d),
                              w=P(d1["n1w"]), b=P(d1["n1b"]), out=P(h1), out_scale=1.0)
    assert lib.mmt_op_prompt_expand_ln(ctypes.byref(la), _stream()) == 0
    torch.cuda.synchronize()
    for name, t, n in (("a8_0", a8_0, B * L), ("c8_0", c8_0, B * L), ("X0", X0, B * L), ("h0", h0, B * L),
                       ("l0", l0, B * L), ("fs0", fs0, B), ("a8_1", a8_1, B * L), ("c8_1", c8_1, B * L),
                       ("X1", X1, B * Na), ("h1", h1, B * Na), ("fs1", fs1, B), ("X1_mid", X1_mid, B * Na)):
        check_guard(t, n, name)
        r[name] = t[:n].cpu()
    r.update(keep=keep, Na=Na, gidx=gidx, s2p=s2p, X1_in=X1_in[:B * Na].cpu(), ws=ws, bias=bias)
    return r


_PIPE = {}


def pipeline(lib, W, case, big_smooth):
    """One run per case with nothing forced, shared by the value tests (the results are not modified)."""
    key = (case, big_smooth)
    if key not in _PIPE:
        _PIPE[key] = run_pipeline(lib, W, *case, big_smooth=big_smooth)
    return _PIPE[key]


def fovea_stats_ref(a8, sm, Lz):
    """[B][32]: per part (template slots, search slots) the channel maxima of a8 * smooth, then the sums of exp."""
    v = a8 * sm
    out = []
    for part in (v[:, :Lz], v[:, Lz:]):
        m = part.max(dim=1).values
        out += [m, torch.exp(part - m[:, None]).sum(1)]
    return torch.cat(out, dim=1)


def fovea_ref(a8, sm, Lz):
    v = a8 * sm
    return torch.cat([torch.softmax(v[:, :Lz], 1), torch.softmax(v[:, Lz:], 1)], 1) * a8


def ln(x, w, b):
    return F.layer_norm(x, (C,), w, b, EPS)


def stage_refs(r, W, dt):
    """Every stage's reference in dtype dt (float64: the reference; float32: the yardstick of the 8 x rule) on the
    fp32 inputs the kernel had -- later stages take the kernel's own a8 / c8 of the stage before."""
    c = lambda t: t.to(dt)
    w0, w1 = {k: c(v) for k, v in W[0].items() if torch.is_tensor(v)}, {k: c(v) for k, v in W[1].items() if torch.is_tensor(v)}
    B, Lz, Lx = r["B"], r["Lz"], r["Lx"]
    L, Na = Lz + Lx, r["Na"]
    o = {}
    lnA, lnB = ln(c(r["tok_rgb"]), w0["ng"], w0["nb"]), ln(c(r["tok_aux"]), w0["ng"], w0["nb"])
    o["lnA0"], o["lnB0"] = lnA, lnB
    o["a8_0"], o["c8_0"] = lnA @ w0["w00"].t() + w0["b00"], lnB @ w0["w01"].t() + w0["b01"]
    a8, c8 = c(r["a8_0"]).reshape(B, L, 8), c(r["c8_0"]).reshape(B, L, 8)
    s8 = fovea_ref(a8, r["sm0"], Lz) + c8
    o["s8_0"] = s8
    o["X0"] = ((c(r["tok_rgb"]).reshape(B, L, C) + (s8 @ w0["V"].t() + w0["v0"])) + c(r["pos"])).reshape(B * L, C)
    o["fs0"] = fovea_stats_ref(a8, r["sm0"], Lz)
    # deep layer 1: a8 from the recovered X (zero rows at pruned slots), c8 through the unfolded chain
    xin = c(r["X1_mid"]).reshape(B, Na, C)
    rec = torch.zeros(B, L, C, dtype=dt)
    rec[:, :Lz] = xin[:, :Lz]
    for b in range(B):
        rec[b, Lz + r["gidx"][b].long()] = xin[b, Lz:]
    o["lnA1"] = ln(rec, w0["ng"], w0["nb"]).reshape(B * L, C)
    o["a8_1"] = o["lnA1"] @ w1["w00"].t() + w1["b00"]
    o["lnB1"] = ln(s8 @ w0["V"].t() + w0["v0"], w1["ng"], w1["nb"]).reshape(B * L, C)
    o["c8_1"] = o["lnB1"] @ w1["w01"].t() + w1["b01"]
    a8, c8 = c(r["a8_1"]).reshape(B, L, 8), c(r["c8_1"]).reshape(B, L, 8)
    s8 = fovea_ref(a8, r["sm1"], Lz) + c8
    o["s8_1"] = s8
    Pm = s8 @ w1["V"].t() + w1["v0"]
    slot = torch.cat([torch.arange(Lz).expand(B, Lz), Lz + r["gidx"].long()], 1)
    o["X1"] = (xin + torch.gather(Pm, 1, slot[:, :, None].expand(B, Na, C))).reshape(B * Na, C)
    o["fs1"] = fovea_stats_ref(a8, r["sm1"], Lz)
    o["slot"] = slot
    return o


_REFS = {}


def refs(lib, W, case, big_smooth):
    key = (case, big_smooth)
    if key not in _REFS:
        r = pipeline(lib, W, case, big_smooth)
        _REFS[key] = (stage_refs(r, W, torch.float64), stage_refs(r, W, torch.float32))
    return _REFS[key]


def check_8x(name, got, r64, r32, floor):
    """The kernel may be 8 x as far from float64 as the same formula in fp32 torch, floored at `floor` (a derived
    rounding bar of the output, elementwise); prints the errors and their ratio."""
    e_k, e_t = (got.double() - r64).abs(), (r32.double() - r64).abs().max().item()
    ratio = e_k.max().item() / e_t if e_t > 0 else float("inf") if e_k.max().item() > 0 else 0.0
    print(f"{name}: kernel max |err| {e_k.max().item():.3e}, fp32 reference {e_t:.3e}, ratio {ratio:.2f}, "
          f"floor (max) {floor.max().item():.3e}")
    allowed = torch.maximum(torch.full_like(e_k, 8 * e_t), floor.expand_as(e_k))
    assert (e_k <= allowed).all(), f"{name}: {e_k.max().item():.3e} > 8 x {e_t:.3e}"
    return allowed.max().item()


def dot_bar(lnv, Wm, bias):
    """(768 + 16) 2^-24 sum |a_i b_i| of a 768-long fp32 dot product in unspecified order, plus the LayerNorm bar
    (rtol = atol = 1e-4) of its left operand propagated through sum |w|."""
    return (C + 16) * U * (lnv.abs() @ Wm.abs().t() + bias.abs()) + (1e-4 + 1e-4 * lnv.abs()) @ Wm.abs().t()


def ln_out_bar(ref_ln, x64, w, dX, rtol, atol):
    """The LN bar on a row whose input is off by at most dX: |d xhat_i| <= rstd dX (2 + |xhat_i|)."""
    xc = x64 - x64.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xc.pow(2).mean(-1, keepdim=True) + EPS)
    return atol + rtol * ref_ln.abs() + w.abs() * rstd * (2 + (xc * rstd).abs()) * dX


SMOOTH = [False, True, "flat"]


@pytest.mark.parametrize("case", CASES)
def test_prompt_reduce_layer0_values(lib, W, case):
    """a8 = conv0_0(LN_A(tok_rgb)), c8 = conv0_1(LN_B(tok_aux)) against float64 at the derived dot-product bar."""
    r, (r64, _) = pipeline(lib, W, case, False), refs(lib, W, case, False)
    w0 = {k: v.double() for k, v in W[0].items() if torch.is_tensor(v)}
    for name, lnv, Wm, bias in (("a8_0", r64["lnA0"], w0["w00"], w0["b00"]), ("c8_0", r64["lnB0"], w0["w01"], w0["b01"])):
        err, bar = (r[name].double() - r64[name]).abs(), dot_bar(lnv, Wm, bias)
        print(f"layer 0 {name} {case}: max |err| {err.max().item():.3e}, max err / bar {(err / bar).max().item():.3e}")
        assert (err <= bar).all()


@pytest.mark.parametrize("big_smooth", SMOOTH)
@pytest.mark.parametrize("case", CASES)
def test_prompt_expand_ln_mode1_values(lib, W, case, big_smooth):
    """X = (tok_rgb + conv1x1(fovea(a8) + c8)) + pos, LN1(X) in hi / lo halves and the fovea statistics."""
    r, (r64, r32) = pipeline(lib, W, case, big_smooth), refs(lib, W, case, big_smooth)
    Lz, Lx, B = case
    w0 = {k: v.double() for k, v in W[0].items() if torch.is_tensor(v)}
    terms = (r64["s8_0"].abs() @ w0["V"].abs().t() + w0["v0"].abs()).reshape(-1, C) + r["tok_rgb"].double().abs() \
        + r["pos"].double().abs().repeat(B, 1)
    dX = check_8x(f"mode-1 X {case} smooth {r['sm0']:.2f}", r["X0"], r64["X0"], r32["X0"], 24 * U * terms)
    check_fstat(f"mode-1 fstat {case} smooth {r['sm0']:.2f}", r["fs0"], r64["fs0"], r32["fs0"], Lz, Lx)
    ref_ln = ln(r64["X0"], w0["n1w"], w0["n1b"])
    got = (r["h0"].double() + r["l0"].double()) / 256.0
    bar = ln_out_bar(ref_ln, r64["X0"], w0["n1w"], dX, 1e-4, 1e-4)
    assert ((got - ref_ln).abs() <= bar).all()


def check_fstat(name, got, r64, r32, Lz, Lx):
    """Channel maxima: one fp32 product, floor 2 ulp; sums of exp over n slots: floor (n + 16) 2^-24 sum."""
    n = torch.tensor([Lz] * 8 + [Lx] * 8, dtype=torch.float64)
    floor = torch.cat([2 * U * r64[:, 0:8].abs(), (n[:8] + 16) * U * r64[:, 8:16], 2 * U * r64[:, 16:24].abs(),
                       (n[8:] + 16) * U * r64[:, 24:32]], 1)
    check_8x(name, got, r64, r32, floor)


@pytest.mark.parametrize("big_smooth", SMOOTH)
@pytest.mark.parametrize("case", CASES)
def test_prompt_reduce_deep_values(lib, W, case, big_smooth):
    """Deep a8 from the folded conv0_0 on the recovered X (a pruned slot gives b00f exactly), c8 through the
    PromptFold against the unfolded chain conv0_1(LN_B(conv1x1_prev(fovea(a8p) + c8p)))."""
    r, (r64, r32) = pipeline(lib, W, case, big_smooth), refs(lib, W, case, big_smooth)
    Lz, Lx, B = case
    w1 = {k: v.double() for k, v in W[1].items() if torch.is_tensor(v)}
    err, bar = (r["a8_1"].double() - r64["a8_1"]).abs(), dot_bar(r64["lnA1"], w1["w00"], w1["b00"])
    print(f"deep a8 {case}: max |err| {err.max().item():.3e}, max err / bar {(err / bar).max().item():.3e}")
    assert (err <= bar).all()
    pruned = torch.cat([torch.zeros(B, Lz, dtype=torch.bool), r["s2p"] < 0], 1).reshape(-1)
    assert pruned.any() and (r["a8_1"][pruned] == W[1]["b00f"]).all()
    floor = (C + 16) * U * (r64["lnB1"].abs() @ w1["w01"].abs().t() + w1["b01"].abs())
    check_8x(f"deep c8 {case} smooth {r['sm0']:.2f}", r["c8_1"], r64["c8_1"], r32["c8_1"], floor)
    assert torch.equal(r["X1_mid"], r["X1_in"])   # no RowReduce: X is read only


@pytest.mark.parametrize("big_smooth", SMOOTH)
@pytest.mark.parametrize("case", CASES)
def test_prompt_expand_ln_mode2_values(lib, W, case, big_smooth):
    """X += conv1x1(fovea(a8) + c8)[slot], slot = t < Lz ? t : Lz + gidx[t - Lz] with a shuffled, shortened gidx;
    LN1(X) in bf16 and the statistics."""
    r, (r64, r32) = pipeline(lib, W, case, big_smooth), refs(lib, W, case, big_smooth)
    Lz, Lx, B = case
    w1 = {k: v.double() for k, v in W[1].items() if torch.is_tensor(v)}
    Pt = r64["s8_1"].abs() @ w1["V"].abs().t() + w1["v0"].abs()
    terms = torch.gather(Pt, 1, r64["slot"][:, :, None].expand(B, r["Na"], C)).reshape(-1, C) + r["X1_mid"].double().abs()
    dX = check_8x(f"mode-2 X {case} smooth {r['sm1']:.2f}", r["X1"], r64["X1"], r32["X1"], 24 * U * terms)
    check_fstat(f"mode-2 fstat {case} smooth {r['sm1']:.2f}", r["fs1"], r64["fs1"], r32["fs1"], Lz, Lx)
    ref_ln = ln(r64["X1"], w1["n1w"], w1["n1b"])
    bar = ln_out_bar(ref_ln, r64["X1"], w1["n1w"], dX, 1e-2, 1e-2)
    assert ((r["h1"].double() - ref_ln).abs() <= bar).all()
    # the bf16 row is the rounding of LN of the X the kernel wrote, within the LN bar
    mine = ln(r["X1"].double(), w1["n1w"], w1["n1b"])
    assert ((r["h1"].double() - mine).abs() <= 2.0 ** -8 * mine.abs() + 1e-4 + 1e-4 * mine.abs()).all()


# --------------------------------------------------------------------------------------------- bitwise: partition, hand-off
PIPE_KEYS = ("a8_0", "c8_0", "X0", "h0", "l0", "fs0", "a8_1", "c8_1", "X1_mid", "X1", "h1", "fs1")


@pytest.mark.parametrize("Lz,Lx", GEOS)
def test_block_partition_bitwise(lib, W, Lz, Lx):
    """"Every block that needs a sequence's statistics forms the same bits": deep prompt_reduce and prompt_expand_ln
    (both modes) with 1, 2 and 4 slots per wave give bit-identical a8, c8, X, LN rows and statistics -- also against
    the unforced run (B = 2: one slot per wave) and across the register / LDS branches of the fovea reduction."""
    B = 2
    base = pipeline(lib, W, (Lz, Lx, B), False) if (Lz, Lx, B) in CASES else run_pipeline(lib, W, Lz, Lx, B)
    try:
        for R in (1, 2, 4):
            assert lib.mmt_tokens_force_config(R, -1) == 0
            r = run_pipeline(lib, W, Lz, Lx, B)
            for k in PIPE_KEYS:
                assert torch.equal(r[k], base[k]), (R, k)
    finally:
        lib.mmt_tokens_force_config(-1, -1)


@pytest.mark.parametrize("Lz,Lx", GEOS)
def test_fstat_handoff_bitwise(lib, W, Lz, Lx):
    """fstat_p as the previous layer's LN1 wrote it gives "the same bits" as the statistics re-reduced by the deep
    prompt kernel (fstat_p = NULL)."""
    B = 3
    a, b = run_pipeline(lib, W, Lz, Lx, B, use_fstat=True), run_pipeline(lib, W, Lz, Lx, B, use_fstat=False)
    for k in PIPE_KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("ks", [1, 2, 3, 8])
def test_row_reduce_deep_prompt(lib, W, ks):
    """The deep prompt kernel applies the pending fc2 update to the live rows of X and writes them back: the bits of
    the reduce arithmetic; a8 / c8 are those of a run on the reduced X."""
    Lz, Lx, B = 64, 257, 2
    r = run_pipeline(lib, W, Lz, Lx, B, ks=ks)
    want = reduced(r["X1_in"].cuda(), r["ws"], 0.25, r["bias"]).cpu()
    assert torch.equal(r["X1_mid"], want)   # every compact row is live (template rows and the kept slots)
    from mmtrack_amd import _lib
    d1 = W["dev"][1]
    L, Na = Lz + Lx, r["Na"]
    X, a8, c8 = want.cuda(), nan_rows(B * L, 8), nan_rows(B * L, 8)
    a8p, c8p, s2p = r["a8_0"].cuda(), r["c8_0"].cuda(), r["s2p"].cuda()
    a = _lib.MmtPromptArgs(layer=1, B=B, Lz=Lz, Lx=Lx, srcA=P(X), srcA_rows=Na, slot2pos=P(s2p), w00=P(d1["w00f"]),
                           b00=P(d1["b00f"]), fold=P(d1["fold"]), a8=P(a8), c8=P(c8), a8p=P(a8p), c8p=P(c8p),
                           smooth_p=r["sm0"], fstat_p=None)
    assert lib.mmt_op_prompt_reduce(ctypes.byref(a), None, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(a8[:B * L].cpu(), r["a8_1"]) and torch.equal(c8[:B * L].cpu(), r["c8_1"])
    ws9 = torch.zeros(9, 1, C, device="cuda")
    a8n = nan_rows(B * L, 8)
    a.a8 = P(a8n)
    assert lib.mmt_op_prompt_reduce(ctypes.byref(a), reduce_arg(ws9, 0.25, r["bias"]), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(a8n).all()


def test_prompt_rejects(lib, W):
    """Lz + Lx > 1024 (the fovea staging holds 1 024 slots): MMT_E_ARG from both prompt entry points, nothing launched."""
    from mmtrack_amd import _lib
    d1 = W["dev"][1]
    t = nan_rows(8, 8)
    a = _lib.MmtPromptArgs(layer=1, B=1, Lz=256, Lx=769, srcA=P(t), srcA_rows=1025, slot2pos=P(t), w00=P(d1["w00f"]),
                           b00=P(d1["b00f"]), fold=P(d1["fold"]), a8=P(t), c8=P(t), a8p=P(t), c8p=P(t), smooth_p=1.0)
    assert lib.mmt_op_prompt_reduce(ctypes.byref(a), None, _stream()) == -1
    la = _lib.MmtLnPromptArgs(mode=1, rows=1025, rows_per_seq=1025, Lz=256, Lx=769, X=P(t), a8=P(t), c8=P(t), smooth=1.0,
                              w1=P(d1["w1t"]), b1=P(d1["v0"]), tok_rgb=P(t), pos=P(t), w=P(d1["n1w"]), b=P(d1["n1b"]),
                              out=P(t), out_scale=1.0)
    assert lib.mmt_op_prompt_expand_ln(ctypes.byref(la), _stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(t).all()
