// The engine's weights: the reference state_dict layout it expects, the f16x3 range scales and their bounds, BN and
// prompt folding, and the packing of it all into one HBM arena.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "engine.h"

using namespace mmt;

namespace {

// -- bf16 round-to-nearest-even on the host (finite inputs)
inline uint16_t host_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

void add_expected(mmt_engine* e, const std::string& k, std::vector<int64_t> shape) {
  e->expected[k] = std::move(shape);
  e->expected_order.push_back(k);
}

}  // namespace

// Reference state_dict layout (ostrack_prompt.py:94-145 / vit_ce_prompt.py:84-182 / ostrack.py:95-144).
void mmt::build_expected(mmt_engine* e) {
  const auto& c = e->cfg;
  const bool vipt = c.model == MMT_MODEL_VIPT;
  add_expected(e, "backbone.cls_token", {1, 1, C});
  add_expected(e, "backbone.pos_embed", {1, 197, C});
  add_expected(e, "backbone.pos_embed_z", {1, e->Lz, C});
  add_expected(e, "backbone.pos_embed_x", {1, e->Lx, C});
  add_expected(e, "backbone.patch_embed.proj.weight", {C, 3, 16, 16});
  add_expected(e, "backbone.patch_embed.proj.bias", {C});
  if (vipt) {
    add_expected(e, "backbone.patch_embed_prompt.proj.weight", {C, 3, 16, 16});
    add_expected(e, "backbone.patch_embed_prompt.proj.bias", {C});
    for (int i = 0; i < e->nprompt; ++i) {
      const std::string p = "backbone.prompt_blocks." + std::to_string(i) + ".";
      add_expected(e, p + "conv0_0.weight", {8, C, 1, 1});
      add_expected(e, p + "conv0_0.bias", {8});
      add_expected(e, p + "conv0_1.weight", {8, C, 1, 1});
      add_expected(e, p + "conv0_1.bias", {8});
      add_expected(e, p + "conv1x1.weight", {C, 8, 1, 1});
      add_expected(e, p + "conv1x1.bias", {C});
      add_expected(e, p + "fovea.smooth", {1});
      add_expected(e, "backbone.prompt_norms." + std::to_string(i) + ".weight", {C});
      add_expected(e, "backbone.prompt_norms." + std::to_string(i) + ".bias", {C});
    }
  }
  for (int i = 0; i < DEPTH; ++i) {
    const std::string p = "backbone.blocks." + std::to_string(i) + ".";
    add_expected(e, p + "norm1.weight", {C});
    add_expected(e, p + "norm1.bias", {C});
    add_expected(e, p + "attn.qkv.weight", {3 * C, C});
    add_expected(e, p + "attn.qkv.bias", {3 * C});
    add_expected(e, p + "attn.proj.weight", {C, C});
    add_expected(e, p + "attn.proj.bias", {C});
    add_expected(e, p + "norm2.weight", {C});
    add_expected(e, p + "norm2.bias", {C});
    add_expected(e, p + "mlp.fc1.weight", {MLPD, C});
    add_expected(e, p + "mlp.fc1.bias", {MLPD});
    add_expected(e, p + "mlp.fc2.weight", {C, MLPD});
    add_expected(e, p + "mlp.fc2.bias", {C});
  }
  add_expected(e, "backbone.norm.weight", {C});
  add_expected(e, "backbone.norm.bias", {C});
  const int hc = c.head_channels;
  const int ch[5] = {C, hc, hc / 2, hc / 4, hc / 8};
  const char* br[3] = {"ctr", "offset", "size"};
  const int n5[3] = {1, 2, 2};
  for (int b = 0; b < 3; ++b) {
    for (int j = 1; j <= 4; ++j) {
      const std::string p = std::string("box_head.conv") + std::to_string(j) + "_" + br[b] + ".";
      add_expected(e, p + "0.weight", {ch[j], ch[j - 1], 3, 3});
      add_expected(e, p + "0.bias", {ch[j]});
      add_expected(e, p + "1.weight", {ch[j]});
      add_expected(e, p + "1.bias", {ch[j]});
      add_expected(e, p + "1.running_mean", {ch[j]});
      add_expected(e, p + "1.running_var", {ch[j]});
      add_expected(e, p + "1.num_batches_tracked", {});
    }
    add_expected(e, std::string("box_head.conv5_") + br[b] + ".weight", {n5[b], ch[4], 1, 1});
    add_expected(e, std::string("box_head.conv5_") + br[b] + ".bias", {n5[b]});
  }
  add_expected(e, "output_window", {1, 1, e->fs, e->fs});  // hann2d (vipt.py:30), computed by the caller
}

namespace {

template <class T>
T* walloc(mmt_engine* e, size_t n) {
  size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
  if (e->wused + bytes > e->wcap) return nullptr;
  T* p = reinterpret_cast<T*>(static_cast<char*>(e->warena) + e->wused);
  e->wused += bytes;
  return p;
}

const std::vector<float>& H(mmt_engine* e, const std::string& k) { return e->host.at(k).data; }

int upload_f32(mmt_engine* e, float** dst, const std::vector<float>& v) {
  *dst = walloc<float>(e, v.size());
  if (!*dst) return e->fail(MMT_E_HIP, "weight arena overflow");
  HIPCHECK(e, hipMemcpy(*dst, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  return MMT_OK;
}
// ---- f16x3 range scales (common.h): the power of two s with bound * s <= 2^14, so the fp16 halves of
// every value * s stay finite and normal down to bound * 2^-28
float range_scale(double bound) {
  if (!(bound > 0) || !std::isfinite(bound)) return 1.0f;
  const int ex = std::min(std::max((int)std::ceil(std::log2(bound)), -60), 60);
  return std::ldexp(1.0f, 14 - ex);
}
inline uint16_t host_f16(float f) {   // RNE, finite inputs within the fp16 range
  const _Float16 h = (_Float16)f;
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}
inline float host_f16f(uint16_t u) {
  _Float16 h;
  std::memcpy(&h, &u, 2);
  return (float)h;
}
double max_abs(const std::vector<float>& v) {
  double m = 0;
  for (float x : v) m = std::max(m, (double)std::fabs(x));
  return m;
}
// bounds of a LayerNorm output y = xhat * g + b (sum xhat^2 <= C): per element, and of the row's 2-norm
double ln_elem_bound(const std::vector<float>& g, const std::vector<float>& b) {
  return std::sqrt((double)g.size()) * max_abs(g) + max_abs(b);
}
double ln_norm_bound(const std::vector<float>& g, const std::vector<float>& b) {
  double bb = 0;
  for (float x : b) bb += (double)x * x;
  return std::sqrt((double)g.size()) * max_abs(g) + std::sqrt(bb);
}
// max_j |w_j . a + b_j| over inputs with |a|_2 <= anorm (rows of w, K each)
double linear_bound(const std::vector<float>& w, const std::vector<float>& b, size_t K, double anorm) {
  double m = 0;
  for (size_t j = 0; j * K < w.size(); ++j) {
    double n2 = 0;
    for (size_t k = 0; k < K; ++k) n2 += (double)w[j * K + k] * w[j * K + k];
    m = std::max(m, std::sqrt(n2) * anorm + (j < b.size() ? std::fabs((double)b[j]) : 0.0));
  }
  return m;
}

// GEMM weight: bf16 in bf16 mode; in fp32-faithful mode the f16x3 halves of w * s (s = range_scale(max|w|))
int upload_w(mmt_engine* e, bf16_t** dst, bf16_t** dst_lo, const std::vector<float>& v, float* scale = nullptr) {
  std::vector<uint16_t> t(v.size()), tl(v.size());
  const float sc = e->split ? range_scale(max_abs(v)) : 1.0f;
  if (scale) *scale = sc;
  for (size_t i = 0; i < v.size(); ++i) {
    if (e->split) {
      t[i] = host_f16(v[i] * sc);
      tl[i] = host_f16(v[i] * sc - host_f16f(t[i]));
    } else {
      t[i] = host_bf16(v[i]);
    }
  }
  *dst = walloc<bf16_t>(e, v.size());
  if (!*dst) return e->fail(MMT_E_HIP, "weight arena overflow");
  HIPCHECK(e, hipMemcpy(*dst, t.data(), t.size() * 2, hipMemcpyHostToDevice));
  *dst_lo = nullptr;
  if (e->split) {
    *dst_lo = walloc<bf16_t>(e, v.size());
    if (!*dst_lo) return e->fail(MMT_E_HIP, "weight arena overflow");
    HIPCHECK(e, hipMemcpy(*dst_lo, tl.data(), tl.size() * 2, hipMemcpyHostToDevice));
  }
  return MMT_OK;
}

// BN(eval) folded into the preceding conv, weights reordered [out][ky][kx][in] (implicit-GEMM K order).
void fold_conv(mmt_engine* e, const std::string& p, int cout, int cin, std::vector<float>& w_out,
               std::vector<float>& b_out, size_t w_off, size_t b_off) {
  const auto& w = H(e, p + ".0.weight");
  const auto& b = H(e, p + ".0.bias");
  const auto& g = H(e, p + ".1.weight");
  const auto& be = H(e, p + ".1.bias");
  const auto& rm = H(e, p + ".1.running_mean");
  const auto& rv = H(e, p + ".1.running_var");
  for (int o = 0; o < cout; ++o) {
    const double s = (double)g[o] / std::sqrt((double)rv[o] + 1e-5);  // head.py:20 BatchNorm2d eps
    b_out[b_off + o] = (float)(((double)b[o] - (double)rm[o]) * s + (double)be[o]);
    for (int ci = 0; ci < cin; ++ci)
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx)
          w_out[w_off + (size_t)o * 9 * cin + (size_t)(ky * 3 + kx) * cin + ci] =
              (float)((double)w[(((size_t)o * cin + ci) * 3 + ky) * 3 + kx] * s);
  }
}

}  // namespace

// The folded constants of deep prompt layer i (host only, formed in double, stored as fp32), from the raw tensors:
//   w00f / b00f: conv0_0(LN_A(x)) = (W00 diag gA) xhat + (b00 + W00 bA), LN_A = prompt_norms[i-1]
//   fold:        PromptFold (kernels.h) from LN_B = prompt_norms[i], conv0_1 of block i and conv1x1 of block i-1
// W00, W01: [8][768]; V: [768][8]
void mmt::prompt_fold(const float* W00, const float* b00, const float* gA, const float* bA, const float* W,
                      const float* w0, const float* g, const float* bb, const float* V, const float* v0, float* wf,
                      float* bf, float* f) {
  for (int k = 0; k < 8; ++k) {
    double acc = b00[k];
    for (int c = 0; c < C; ++c) {
      wf[(size_t)k * C + c] = (float)((double)W00[(size_t)k * C + c] * gA[c]);
      acc += (double)W00[(size_t)k * C + c] * bA[c];
    }
    bf[k] = (float)acc;
  }
  double cm[8] = {0}, bm = 0;
  for (int c = 0; c < C; ++c) {
    for (int j = 0; j < 8; ++j) cm[j] += V[c * 8 + j];
    bm += v0[c];
  }
  for (int j = 0; j < 8; ++j) cm[j] /= C;
  bm /= C;
  std::vector<double> Vc((size_t)C * 8), vc(C);
  for (int c = 0; c < C; ++c) {
    for (int j = 0; j < 8; ++j) Vc[c * 8 + j] = V[c * 8 + j] - cm[j];
    vc[c] = v0[c] - bm;
  }
  for (int i = 0; i < FOLD_N; ++i) f[i] = 0.f;
  for (int k = 0; k < 8; ++k) {
    double mc = 0, cb = w0[k];
    double Mk[8] = {0};
    for (int c = 0; c < C; ++c) {
      const double wg = (double)W[k * C + c] * g[c];
      for (int j = 0; j < 8; ++j) Mk[j] += wg * Vc[c * 8 + j];
      mc += wg * vc[c];
      cb += (double)W[k * C + c] * bb[c];
    }
    for (int j = 0; j < 8; ++j) f[FOLD_MC + k * 8 + j] = (float)Mk[j];
    f[FOLD_mc + k] = (float)mc;
    f[FOLD_cb + k] = (float)cb;
  }
  double gb = 0;
  for (int j = 0; j < 8; ++j) {
    double gj = 0;
    for (int l = 0; l < 8; ++l) {
      double G = 0;
      for (int c = 0; c < C; ++c) G += Vc[c * 8 + j] * Vc[c * 8 + l];
      f[FOLD_G + j * 8 + l] = (float)(G / C);
    }
    for (int c = 0; c < C; ++c) gj += Vc[c * 8 + j] * vc[c];
    f[FOLD_g + j] = (float)(gj / C);
  }
  for (int c = 0; c < C; ++c) gb += vc[c] * vc[c];
  f[FOLD_gb] = (float)(gb / C);
}

int mmt::pack_weights(mmt_engine* e) {
  const auto& c = e->cfg;
  const bool vipt = c.model == MMT_MODEL_VIPT;
  e->wcap = (e->split ? 400ull : 200ull) << 20;
  HIPCHECK(e, hipMalloc(&e->warena, e->wcap));
  TRY(upload_w(e, &e->pe_w, &e->pe_wl, H(e, "backbone.patch_embed.proj.weight"), &e->pe_s));
  TRY(upload_f32(e, &e->pe_b, H(e, "backbone.patch_embed.proj.bias")));
  if (vipt) {
    TRY(upload_w(e, &e->pep_w, &e->pep_wl, H(e, "backbone.patch_embed_prompt.proj.weight"), &e->pep_s));
    TRY(upload_f32(e, &e->pep_b, H(e, "backbone.patch_embed_prompt.proj.bias")));
  }
  std::vector<float> pos(H(e, "backbone.pos_embed_z"));
  const auto& px = H(e, "backbone.pos_embed_x");
  pos.insert(pos.end(), px.begin(), px.end());
  TRY(upload_f32(e, &e->pos, pos));
  for (int i = 0; i < e->nprompt; ++i) {
    const std::string p = "backbone.prompt_blocks." + std::to_string(i) + ".";
    PromptW& w = e->pw[i];
    TRY(upload_f32(e, &w.w00, H(e, p + "conv0_0.weight")));
    TRY(upload_f32(e, &w.b00, H(e, p + "conv0_0.bias")));
    TRY(upload_f32(e, &w.w01, H(e, p + "conv0_1.weight")));
    TRY(upload_f32(e, &w.b01, H(e, p + "conv0_1.bias")));
    {   // conv1x1 [768][8] stored channel-major [8][768]: the LN1 kernel's LDS image is a straight copy
      const auto& v = H(e, p + "conv1x1.weight");
      std::vector<float> t(v.size());
      for (size_t c = 0; c < (size_t)C; ++c)
        for (size_t k = 0; k < 8; ++k) t[k * C + c] = v[c * 8 + k];
      TRY(upload_f32(e, &w.w1, t));
    }
    TRY(upload_f32(e, &w.b1, H(e, p + "conv1x1.bias")));
    w.smooth = H(e, p + "fovea.smooth")[0];
    TRY(upload_f32(e, &w.nw, H(e, "backbone.prompt_norms." + std::to_string(i) + ".weight")));
    TRY(upload_f32(e, &w.nb, H(e, "backbone.prompt_norms." + std::to_string(i) + ".bias")));
    w.fold = nullptr;
    w.w00f = w.b00f = nullptr;
    if (i >= 1) {   // the deep layers' folded constants (prompt_fold)
      const std::string pp = "backbone.prompt_blocks." + std::to_string(i - 1) + ".";
      std::vector<float> wf((size_t)8 * C), bf(8), f(FOLD_N, 0.f);
      prompt_fold(H(e, p + "conv0_0.weight").data(), H(e, p + "conv0_0.bias").data(),
                  H(e, "backbone.prompt_norms." + std::to_string(i - 1) + ".weight").data(),
                  H(e, "backbone.prompt_norms." + std::to_string(i - 1) + ".bias").data(),
                  H(e, p + "conv0_1.weight").data(), H(e, p + "conv0_1.bias").data(),
                  H(e, "backbone.prompt_norms." + std::to_string(i) + ".weight").data(),
                  H(e, "backbone.prompt_norms." + std::to_string(i) + ".bias").data(),
                  H(e, pp + "conv1x1.weight").data(), H(e, pp + "conv1x1.bias").data(), wf.data(), bf.data(), f.data());
      TRY(upload_f32(e, &w.w00f, wf));
      TRY(upload_f32(e, &w.b00f, bf));
      TRY(upload_f32(e, &w.fold, f));
    }
  }
  for (int i = 0; i < DEPTH; ++i) {
    const std::string p = "backbone.blocks." + std::to_string(i) + ".";
    LayerW& w = e->lw[i];
    TRY(upload_w(e, &w.qkv_w, &w.qkv_wl, H(e, p + "attn.qkv.weight"), &w.qkv_s));
    TRY(upload_f32(e, &w.qkv_b, H(e, p + "attn.qkv.bias")));
    TRY(upload_w(e, &w.proj_w, &w.proj_wl, H(e, p + "attn.proj.weight"), &w.proj_s));
    TRY(upload_f32(e, &w.proj_b, H(e, p + "attn.proj.bias")));
    TRY(upload_w(e, &w.fc1_w, &w.fc1_wl, H(e, p + "mlp.fc1.weight"), &w.fc1_s));
    TRY(upload_f32(e, &w.fc1_b, H(e, p + "mlp.fc1.bias")));
    TRY(upload_w(e, &w.fc2_w, &w.fc2_wl, H(e, p + "mlp.fc2.weight"), &w.fc2_s));
    TRY(upload_f32(e, &w.fc2_b, H(e, p + "mlp.fc2.bias")));
    if (e->split) {   // activation range scales from the weights (bounds: LN outputs, linear layers)
      const auto &g1 = H(e, p + "norm1.weight"), &b1 = H(e, p + "norm1.bias");
      const auto &g2 = H(e, p + "norm2.weight"), &b2 = H(e, p + "norm2.bias");
      w.ln1_s = range_scale(ln_elem_bound(g1, b1));
      w.ln2_s = range_scale(ln_elem_bound(g2, b2));
      w.qkv_os = range_scale(linear_bound(H(e, p + "attn.qkv.weight"), H(e, p + "attn.qkv.bias"), C,
                                          ln_norm_bound(g1, b1)));
      w.fc1_os = range_scale(linear_bound(H(e, p + "mlp.fc1.weight"), H(e, p + "mlp.fc1.bias"), C,
                                          ln_norm_bound(g2, b2)));   // |GELU(h)| <= |h|
    }
    TRY(upload_f32(e, &w.n1w, H(e, p + "norm1.weight")));
    TRY(upload_f32(e, &w.n1b, H(e, p + "norm1.bias")));
    TRY(upload_f32(e, &w.n2w, H(e, p + "norm2.weight")));
    TRY(upload_f32(e, &w.n2b, H(e, p + "norm2.bias")));
  }
  TRY(upload_f32(e, &e->norm_w, H(e, "backbone.norm.weight")));
  TRY(upload_f32(e, &e->norm_b, H(e, "backbone.norm.bias")));
  // head
  const int hc = c.head_channels;
  const int ch[5] = {C, hc, hc / 2, hc / 4, hc / 8};
  const char* br[3] = {"ctr", "offset", "size"};
  {
    std::vector<float> w((size_t)3 * hc * 9 * C), b((size_t)3 * hc);
    for (int k = 0; k < 3; ++k)
      fold_conv(e, std::string("box_head.conv1_") + br[k], hc, C, w, b, (size_t)k * hc * 9 * C, (size_t)k * hc);
    TRY(upload_w(e, &e->hw1, &e->hw1l, w, &e->hw1_s));
    TRY(upload_f32(e, &e->hb1, b));
    if (e->split) {   // head input: final-norm rows; a 3x3 window of them has 2-norm <= 3 * the row bound
      const auto &gn = H(e, "backbone.norm.weight"), &bn = H(e, "backbone.norm.bias");
      e->feat_s = range_scale(ln_elem_bound(gn, bn));
      e->h_s[0] = range_scale(linear_bound(w, b, (size_t)9 * C, 3.0 * ln_norm_bound(gn, bn)));
    }
  }
  for (int j = 2; j <= 4; ++j) {
    const int co = ch[j], ci = ch[j - 1];
    std::vector<float> w((size_t)3 * co * 9 * ci), b((size_t)3 * co);
    for (int k = 0; k < 3; ++k)
      fold_conv(e, std::string("box_head.conv") + std::to_string(j) + "_" + br[k], co, ci, w, b,
                (size_t)k * co * 9 * ci, (size_t)k * co);
    TRY(upload_w(e, &e->hw[j - 2], &e->hwl[j - 2], w, &e->hw_s[j - 2]));
    TRY(upload_f32(e, &e->hb[j - 2], b));
    if (e->split && j < 4) {   // h_{j}: input elements <= 2^14 / h_s[j-2], window 2-norm <= 3 sqrt(ci) of that
      const double in_b = std::ldexp(1.0, 14) / e->h_s[j - 2];
      e->h_s[j - 1] = range_scale(linear_bound(w, b, (size_t)9 * ci, 3.0 * std::sqrt((double)ci) * in_b));
    }
  }
  {
    std::vector<float> w5, b5;
    for (int k = 0; k < 3; ++k) {
      const auto& w = H(e, std::string("box_head.conv5_") + br[k] + ".weight");
      const auto& b = H(e, std::string("box_head.conv5_") + br[k] + ".bias");
      w5.insert(w5.end(), w.begin(), w.end());
      b5.insert(b5.end(), b.begin(), b.end());
    }
    TRY(upload_f32(e, &e->w5, w5));
    TRY(upload_f32(e, &e->b5, b5));
  }
  TRY(upload_f32(e, &e->hann, H(e, "output_window")));
  return MMT_OK;
}
