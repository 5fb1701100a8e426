"""The weight loader's prompt folds (mmt_prompt_fold, host only) against the unfolded chain in float64.

Deep prompt layer i replaces conv0_1(LN_B(conv1x1_prev(s8))) by a quadratic form in the 8-vector s8 (PromptFold,
csrc/kernels.h) and conv0_0(LN_A(x)) by conv0_0 with LN_A's affine folded in.  Both are formed in double and stored
as fp32, so evaluated in float64 from the stored numbers only the fp32 rounding of those constants separates them
from the unfolded reference: each constant is off by at most 2^-24 relative, an output's error is at most 2^-24 times
the sum of the magnitudes of its terms, and the bar is 160 times that (160 = the constants of one fold).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mmtrack_amd import _lib, synth

C = 768
EPS = 1e-6
U = 2.0 ** -24
FOLD_MC, FOLD_mc, FOLD_cb, FOLD_G, FOLD_g, FOLD_gb, FOLD_N = 0, 64, 72, 80, 144, 152, 160


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(0, kind="vipt", prompt_type="vipt_deep")


def fold_layer(sd, i):
    """mmt_prompt_fold on layer i's raw fp32 tensors -> (w00f [8][768], b00f [8], fold [160]) as float32 arrays."""
    lib = _lib.load()
    p, pp = f"backbone.prompt_blocks.{i}.", f"backbone.prompt_blocks.{i - 1}."
    ins = [sd[p + "conv0_0.weight"], sd[p + "conv0_0.bias"], sd[f"backbone.prompt_norms.{i - 1}.weight"],
           sd[f"backbone.prompt_norms.{i - 1}.bias"], sd[p + "conv0_1.weight"], sd[p + "conv0_1.bias"],
           sd[f"backbone.prompt_norms.{i}.weight"], sd[f"backbone.prompt_norms.{i}.bias"], sd[pp + "conv1x1.weight"],
           sd[pp + "conv1x1.bias"]]
    ins = [np.ascontiguousarray(t.numpy().astype(np.float32).reshape(-1)) for t in ins]
    wf, bf, fo = np.zeros(8 * C, np.float32), np.zeros(8, np.float32), np.full(FOLD_N, np.nan, np.float32)
    rc = lib.mmt_prompt_fold(*[a.ctypes.data_as(ctypes.c_void_p) for a in ins + [wf, bf, fo]])
    assert rc == 0
    return wf.reshape(8, C), bf, fo


def s8_cases(sd, i, g):
    """Random s8 at three magnitudes, plus directions scaled so that |V's| = |v0'| (the LN_B variance form
    s'Gs + 2 g.s + gb cancels most there), the least-squares s8 = -argmin |V's + v0'| among them."""
    V = sd[f"backbone.prompt_blocks.{i - 1}.conv1x1.weight"].double().reshape(C, 8)
    v0 = sd[f"backbone.prompt_blocks.{i - 1}.conv1x1.bias"].double()
    Vc, vc = V - V.mean(0, keepdim=True), v0 - v0.mean()
    r = torch.randn(24, 8, generator=g, dtype=torch.float64)
    out = [r[:8] * 0.1, r[8:16], r[16:24] * 10.0]
    d = torch.randn(16, 8, generator=g, dtype=torch.float64)
    out.append(d * (vc.norm() / (d @ Vc.t()).norm(dim=1, keepdim=True)))
    ls = -torch.linalg.lstsq(Vc, vc[:, None]).solution[:, 0]
    out.append(torch.stack([ls, ls * (vc.norm() / (Vc @ ls).norm())]))
    return torch.cat(out)


@pytest.mark.parametrize("layer", [1, 2])
def test_prompt_fold_c8(sd, layer):
    _, _, fo = fold_layer(sd, layer)
    assert np.isfinite(fo).all()
    f = torch.from_numpy(fo).double()
    Mc, mc, cb = f[FOLD_MC:FOLD_MC + 64].reshape(8, 8), f[FOLD_mc:FOLD_mc + 8], f[FOLD_cb:FOLD_cb + 8]
    G, gg, gb = f[FOLD_G:FOLD_G + 64].reshape(8, 8), f[FOLD_g:FOLD_g + 8], f[FOLD_gb]
    s = s8_cases(sd, layer, torch.Generator().manual_seed(100 + layer))
    # c8 through the fold, float64 arithmetic on the stored fp32 constants
    var = torch.einsum("nj,jl,nl->n", s, G, s) + 2.0 * (s @ gg) + gb
    assert (var > 0).all()
    rstd = 1.0 / torch.sqrt(var + EPS)
    lin = s @ Mc.t() + mc
    got = rstd[:, None] * lin + cb
    # the unfolded chain conv0_1(LN_B(conv1x1_prev(s8))) in float64
    p, pp = f"backbone.prompt_blocks.{layer}.", f"backbone.prompt_blocks.{layer - 1}."
    P = F.linear(s, sd[pp + "conv1x1.weight"].double().reshape(C, 8), sd[pp + "conv1x1.bias"].double())
    ln = F.layer_norm(P, (C,), sd[f"backbone.prompt_norms.{layer}.weight"].double(),
                      sd[f"backbone.prompt_norms.{layer}.bias"].double(), EPS)
    ref = F.linear(ln, sd[p + "conv0_1.weight"].double().reshape(8, C), sd[p + "conv0_1.bias"].double())
    # per output: the magnitudes of the terms of its own sum, rstd (Mc s + mc) + cb
    terms = rstd[:, None] * ((s.abs() @ Mc.abs().t()) + mc.abs()) + cb.abs()
    bar = 160.0 * U * terms
    ratio = ((got - ref).abs() / bar).max().item()
    print(f"prompt fold layer {layer}: c8 max |err| {(got - ref).abs().max().item():.3e}, max err / bar {ratio:.3e} "
          f"over {len(s)} s8 (min var {var.min().item():.3e}, gb {gb.item():.3e})")
    assert ratio <= 1.0


@pytest.mark.parametrize("layer", [1, 2])
def test_prompt_fold_a8(sd, layer):
    wf, bf, _ = fold_layer(sd, layer)
    g = torch.Generator().manual_seed(200 + layer)
    x = torch.cat([torch.randn(12, C, generator=g) * 3 + 1, torch.randn(4, C, generator=g) * 0.01 + 50,
                   torch.zeros(1, C)]).double()
    w, b = torch.from_numpy(wf).double(), torch.from_numpy(bf).double()
    xhat = F.layer_norm(x, (C,), None, None, EPS)
    got = xhat @ w.t() + b
    p = f"backbone.prompt_blocks.{layer}."
    ln = F.layer_norm(x, (C,), sd[f"backbone.prompt_norms.{layer - 1}.weight"].double(),
                      sd[f"backbone.prompt_norms.{layer - 1}.bias"].double(), EPS)
    ref = F.linear(ln, sd[p + "conv0_0.weight"].double().reshape(8, C), sd[p + "conv0_0.bias"].double())
    bar = 160.0 * U * (xhat.abs() @ w.abs().t() + b.abs())
    ratio = ((got - ref).abs() / bar).max().item()
    print(f"prompt fold layer {layer}: a8 max |err| {(got - ref).abs().max().item():.3e}, max err / bar {ratio:.3e}")
    assert ratio <= 1.0
    # the zero row: LN of it is LN_A's bias, so a8 = b00f
    assert torch.allclose(got[-1], b, rtol=0, atol=0)


def test_prompt_fold_rejects_null():
    lib = _lib.load()
    z = np.zeros(8 * C, np.float32)
    ptr = z.ctypes.data_as(ctypes.c_void_p)
    assert lib.mmt_prompt_fold(*([ptr] * 12 + [None])) == _lib.MMT_E_ARG
