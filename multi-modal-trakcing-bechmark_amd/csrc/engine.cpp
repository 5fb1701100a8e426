// Host runtime of the MI355X tracking engine: weight packing, HBM layout, the per-frame launch
// sequence (optionally one hipGraph per batch shape), tracker state and the C ABI of mmtrack.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mmtrack.h"
#include "kernels.h"

using namespace mmt;

namespace {

constexpr int C = 768;
constexpr int HEADS = 12;
constexpr int DEPTH = 12;
constexpr int MLPD = 3072;

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// -- bf16 round-to-nearest-even on the host (finite inputs)
inline uint16_t host_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16) | ((u & 0xffff) ? 0x40 : 0);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

struct LayerW {
  bf16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
  bf16_t *qkv_wl, *proj_wl, *fc1_wl, *fc2_wl;   // low halves (fp32-faithful mode)
  float *qkv_b, *proj_b, *fc1_b, *fc2_b, *n1w, *n1b, *n2w, *n2b;
  // f16x3 range scales (powers of two, 1 in bf16 mode): weights, and the split activations this block
  // produces -- LN1 / LN2 outputs, qkv output (Q, K, V and the attention output O), fc1 (GELU) output
  float qkv_s = 1, proj_s = 1, fc1_s = 1, fc2_s = 1, ln1_s = 1, ln2_s = 1, qkv_os = 1, fc1_os = 1;
};
constexpr int64_t kSplitKWsElems = 4 << 20;   // 16 MB of fp32 split-K partials (mmt_op_gemm)

struct PromptW {
  float *w00, *b00, *w01, *b01, *w1, *b1, *nw, *nb;
  float* fold;   // deep layers: PromptFold (kernels.h) of LN_B + conv0_1 over the previous s8
  float *w00f, *b00f;   // deep layers: conv0_0 with the affine of LN_A (prompt_norms[i-1]) folded in
  float smooth;
};

struct GraphEntry {
  hipGraphExec_t exec = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;   // probe events captured as graph nodes
  std::vector<std::pair<double, double>> work;         // flops / bytes of each bracketed launch
};

struct TimingProbe {
  std::string cls;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;  // eager pool
  size_t used = 0;
  long launches = 0;
  double total_ms = 0, flops = 0, bytes = 0;
  std::vector<std::pair<double, double>> pending_work;  // flops/bytes of each pending pair
  GraphEntry* capture = nullptr;                        // set while capturing a graph
};

}  // namespace

constexpr int kRing = MMT_PIPELINE_DEPTH;   // submitted-but-unfetched frames an engine holds

struct mmt_engine {
  mmt_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  static constexpr int kMaxParts = 4;
  hipStream_t xstream[kMaxParts - 1] = {};   // parts 1.. of a split launch (part 0 runs on `stream`)
  hipEvent_t fork_ev = nullptr, join_ev[kMaxParts - 1] = {};
  int nparts = 2;                      // parts of a split launch (MMT_NPARTS, 2..4)
  int conc_parts = 1;                  // parts of the launch being enqueued (GemmArgs::conc: they share the chip)
  int overlap_min = 64;                // split launches of >= this many sequences over two streams (0: never)
  std::string err;
  std::map<std::string, std::vector<int64_t>> expected;
  std::vector<std::string> expected_order;
  std::map<std::string, HostTensor> host;
  bool finalized = false;

  // geometry
  int Lz = 0, Lx = 0, L = 0, fs = 0, tfs = 0;
  std::vector<int> ls_before;   // search tokens entering block i
  std::vector<int> keep_at;     // search tokens kept after block i (== ls_before[i] if no CE)

  // weights (one arena)
  void* warena = nullptr;
  size_t wcap = 0, wused = 0;
  LayerW lw[DEPTH];
  PromptW pw[DEPTH];
  int nprompt = 0;
  bf16_t *pe_w = nullptr, *pep_w = nullptr, *pe_wl = nullptr, *pep_wl = nullptr;
  float *pe_b = nullptr, *pep_b = nullptr, *pos = nullptr, *norm_w = nullptr, *norm_b = nullptr;
  bf16_t *hw1 = nullptr, *hw1l = nullptr;
  float* hb1 = nullptr;
  bf16_t* hw[3] = {};   // conv2..4, [3 branches] contiguous
  bf16_t* hwl[3] = {};
  float* hb[3] = {};
  // f16x3 range scales: patch-embed weights, head conv weights, final-norm output (head input) and the
  // head's split intermediates h1..h3
  float pe_s = 1, pep_s = 1, hw1_s = 1, hw_s[3] = {1, 1, 1}, feat_s = 1, h_s[3] = {1, 1, 1};
  float *w5 = nullptr, *b5 = nullptr, *hann = nullptr;

  // activations (max_batch)
  void* aarena = nullptr;
  bf16_t *A_rgb = nullptr, *A_aux = nullptr, *Hn = nullptr, *QKV = nullptr, *O = nullptr, *Hm = nullptr,
         *feat = nullptr, *h1 = nullptr, *h2 = nullptr, *h3 = nullptr;
  // low halves of every bf16 GEMM operand (fp32-faithful mode only, else null)
  bf16_t *A_rgb_l = nullptr, *A_aux_l = nullptr, *Hn_l = nullptr, *QKV_l = nullptr, *O_l = nullptr, *Hm_l = nullptr,
         *feat_l = nullptr, *h1_l = nullptr, *h2_l = nullptr, *h3_l = nullptr, *zero = nullptr;
  bool split = false;
  // parity diagnostics (debug_outputs): CE keys by slot [B][n_ce][Lx] as computed, and teacher-forced keys
  float *ce_keys = nullptr, *ce_forced = nullptr;
  bool force_ce = false;
  // a8 / c8: the prompt blocks' two 8-channel branches, [2][B][L][8] each (layer i writes half i & 1 and the
  // next layer re-forms the fovea output s8 from the half it did not write)
  float *tok_rgb = nullptr, *tok_aux = nullptr, *X = nullptr, *X2 = nullptr,
        *a8 = nullptr,
        *c8 = nullptr, *fstat = nullptr, *h4 = nullptr, *ce_prob = nullptr, *res = nullptr, *dbg_maps = nullptr,
        *dbg_feat = nullptr;
  int *gidx0 = nullptr, *gidx1 = nullptr, *slot2pos = nullptr, *gather = nullptr, *removed = nullptr;
  // mask mode (cfg.ce_template_index = MMT_CE_TEMPLATE_MASK): per slot, the compact ascending list of the template
  // tokens whose attention rows score the search tokens ([max_batch][Lz]) and its length; every token (ALL) until
  // mmt_set_ce_template_mask.  Fixed device addresses: captured graphs read the lists' current contents.
  bool ce_mask = false;
  int *ce_rows = nullptr, *ce_nrows = nullptr;
  float* splitk_ws = nullptr;   // [kMaxParts launch parts][kSplitKWsElems] fp32 split-K partials (few-tile GEMMs)
  uint8_t* dbg_patch = nullptr;
  CropParam* params_dev = nullptr;
  SeqState* state_dev = nullptr;      // [max_batch] tracker state per slot (device-resident)
  TrackOut* out_dev = nullptr;        // [max_batch] per-launch results
  CropParam* params_host = nullptr;   // pinned [kRing][max_batch]
  TrackOut* outs_host = nullptr;      // pinned [kRing][max_batch]
  // ring hand-off: the geometry kernel reads a launch's frame parameters straight from params_host and
  // the decode kernel writes its results straight into outs_host (device-visible pinned memory), so a
  // step carries no copy launches; the device counts executed launches (hring.ctr) exactly as `launches`
  // does on the host, and a ticket keeps the ring entry (launches % kRing) its launch used
  bool ring_handoff = true;
  RingArgs hring{};
  int64_t launches = 0;

  // pipelined frames (mmt_track_batch_submit / _fetch): ticket t uses ring entry t % kRing
  struct Ticket {
    int64_t id = -1;
    int first = 0, n = 0;
    bool open = false;
    hipEvent_t done = nullptr;
    const GraphEntry* replayed = nullptr;
    int entry = 0;   // params / results ring entry of its launch
  };
  Ticket ring[kRing];
  int64_t next_ticket = 0;
  int unfetched = 0;

  // host-frame staging: per (slot, ring entry) device copies, made on a copy stream so a pipelined
  // frame's PCIe transfer overlaps the compute of the frames before it
  std::vector<uint8_t*> frame_dev;     // [max_batch * kRing]
  std::vector<size_t> frame_cap;
  hipStream_t cstream = nullptr;
  hipEvent_t copy_ev[kRing] = {};
  hipStream_t frame_stream = nullptr;  // caller's stream that produces device frames (mmt_set_frame_stream;
  bool frame_wait = false;             // null = the legacy default stream)
  hipEvent_t frame_ev = nullptr;

  // tracker state (vipt.py:57, 88) in doubles
  std::vector<std::array<double, 4>> state;
  std::vector<char> active;
  int last_batch = 0;

  std::map<std::tuple<int, int, std::string>, GraphEntry> graphs;
  std::unique_ptr<TimingProbe> probe;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
};

namespace {

#define HIPCHECK(e, expr)                                                              \
  do {                                                                                 \
    hipError_t _st = (expr);                                                           \
    if (_st != hipSuccess)                                                             \
      return (e)->fail(MMT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_st)); \
  } while (0)

void add_expected(mmt_engine* e, const std::string& k, std::vector<int64_t> shape) {
  e->expected[k] = std::move(shape);
  e->expected_order.push_back(k);
}

// Reference state_dict layout (ostrack_prompt.py:94-145 / vit_ce_prompt.py:84-182 / ostrack.py:95-144).
void build_expected(mmt_engine* e) {
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

#define TRY(x)                  \
  do {                          \
    int _r = (x);               \
    if (_r != MMT_OK) return _r; \
  } while (0)

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

// The folded constants of deep prompt layer i (host only, formed in double, stored as fp32), from the raw tensors:
//   w00f / b00f: conv0_0(LN_A(x)) = (W00 diag gA) xhat + (b00 + W00 bA), LN_A = prompt_norms[i-1]
//   fold:        PromptFold (kernels.h) from LN_B = prompt_norms[i], conv0_1 of block i and conv1x1 of block i-1
// W00, W01: [8][768]; V: [768][8]
void prompt_fold(const float* W00, const float* b00, const float* gA, const float* bA, const float* W, const float* w0,
                 const float* g, const float* bb, const float* V, const float* v0, float* wf, float* bf, float* f) {
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

int pack_weights(mmt_engine* e) {
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

int alloc_acts(mmt_engine* e) {
  const int B = e->cfg.max_batch, L = e->L, Lx = e->Lx;
  const int S = e->cfg.search_size, Cin = e->cfg.in_chans;
  const int hc = e->cfg.head_channels;
  struct Req { void** p; size_t bytes; };
  std::vector<Req> reqs = {
      {(void**)&e->A_rgb, (size_t)B * L * C * 2},      {(void**)&e->A_aux, (size_t)B * L * C * 2},
      {(void**)&e->tok_rgb, (size_t)B * L * C * 4},    {(void**)&e->tok_aux, (size_t)B * L * C * 4},
      {(void**)&e->X, (size_t)B * L * C * 4},          {(void**)&e->X2, (size_t)B * L * C * 4},
      {(void**)&e->a8, (size_t)2 * B * L * 8 * 4},     {(void**)&e->fstat, (size_t)B * 32 * 4},
      {(void**)&e->c8, (size_t)2 * B * L * 8 * 4},         {(void**)&e->Hn, (size_t)B * L * C * 2},
      {(void**)&e->QKV, (size_t)B * L * 3 * C * 2},    {(void**)&e->O, (size_t)B * L * C * 2},
      {(void**)&e->Hm, (size_t)B * L * MLPD * 2},      {(void**)&e->feat, (size_t)B * Lx * C * 2},
      {(void**)&e->h1, (size_t)B * Lx * 3 * hc * 2},   {(void**)&e->h2, (size_t)B * Lx * 3 * (hc / 2) * 2},
      {(void**)&e->h3, (size_t)B * Lx * 3 * (hc / 4) * 2}, {(void**)&e->h4, (size_t)B * Lx * 3 * 32 * 4},
      {(void**)&e->ce_prob, (size_t)B * HEADS * Lx * 4}, {(void**)&e->res, (size_t)B * 8 * 4},
      {(void**)&e->gidx0, (size_t)B * Lx * 4},         {(void**)&e->gidx1, (size_t)B * Lx * 4},
      {(void**)&e->slot2pos, (size_t)B * Lx * 4},      {(void**)&e->gather, (size_t)B * L * 4},
      {(void**)&e->removed, (size_t)B * Lx * 4},
      {(void**)&e->params_dev, (size_t)B * sizeof(CropParam)},
      {(void**)&e->state_dev, (size_t)B * sizeof(SeqState)}, {(void**)&e->out_dev, (size_t)B * sizeof(TrackOut)},
  };
  reqs.push_back({(void**)&e->zero, 256});
  if (e->ce_mask) {
    reqs.push_back({(void**)&e->ce_rows, (size_t)B * e->Lz * 4});
    reqs.push_back({(void**)&e->ce_nrows, (size_t)B * 4});
  }
  reqs.push_back({(void**)&e->hring.ctr, 256});   // ctr, cur
  reqs.push_back({(void**)&e->splitk_ws, (size_t)mmt_engine::kMaxParts * kSplitKWsElems * 4});
  if (e->split) {
    const std::vector<Req> lo = {
        {(void**)&e->A_rgb_l, (size_t)B * L * C * 2},   {(void**)&e->A_aux_l, (size_t)B * L * C * 2},
        {(void**)&e->Hn_l, (size_t)B * L * C * 2},      {(void**)&e->QKV_l, (size_t)B * L * 3 * C * 2},
        {(void**)&e->O_l, (size_t)B * L * C * 2},       {(void**)&e->Hm_l, (size_t)B * L * MLPD * 2},
        {(void**)&e->feat_l, (size_t)B * Lx * C * 2},   {(void**)&e->h1_l, (size_t)B * Lx * 3 * hc * 2},
        {(void**)&e->h2_l, (size_t)B * Lx * 3 * (hc / 2) * 2}, {(void**)&e->h3_l, (size_t)B * Lx * 3 * (hc / 4) * 2}};
    reqs.insert(reqs.end(), lo.begin(), lo.end());
  }
  if (e->cfg.debug_outputs) {
    const size_t nce = std::max(e->cfg.n_ce, 1);
    reqs.push_back({(void**)&e->ce_keys, (size_t)B * nce * Lx * 4});
    reqs.push_back({(void**)&e->ce_forced, (size_t)B * nce * Lx * 4});
    reqs.push_back({(void**)&e->dbg_patch, (size_t)B * S * S * Cin});
    reqs.push_back({(void**)&e->dbg_maps, (size_t)B * 5 * Lx * 4});
    reqs.push_back({(void**)&e->dbg_feat, (size_t)B * L * C * 4});
  }
  size_t total = 0;
  for (auto& r : reqs) total += (r.bytes + 255) & ~size_t(255);
  HIPCHECK(e, hipMalloc(&e->aarena, total));
  HIPCHECK(e, hipMemset(e->aarena, 0, total));
  size_t off = 0;
  for (auto& r : reqs) {
    *r.p = static_cast<char*>(e->aarena) + off;
    off += (r.bytes + 255) & ~size_t(255);
  }
  if (e->ce_mask) {   // ALL: every template token of every slot
    std::vector<int> rows((size_t)B * e->Lz), nrows(B, e->Lz);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int)(i % e->Lz);
    HIPCHECK(e, hipMemcpy(e->ce_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    HIPCHECK(e, hipMemcpy(e->ce_nrows, nrows.data(), nrows.size() * 4, hipMemcpyHostToDevice));
  }
  // the ring is read / written by kernels in place: fine-grained coherent pinned memory, so no GPU cache
  // holds a stale copy of an entry between the launches that reuse it (frame pointer / size may change)
  constexpr unsigned kRingFlags = hipHostMallocMapped | hipHostMallocCoherent;
  HIPCHECK(e, hipHostMalloc((void**)&e->params_host, (size_t)kRing * B * sizeof(CropParam), kRingFlags));
  HIPCHECK(e, hipHostMalloc((void**)&e->outs_host, (size_t)kRing * B * sizeof(TrackOut), kRingFlags));
  e->hring.cur = e->hring.ctr + 1;
  e->hring.kring = kRing;
  e->hring.pitch = B;
  e->ring_handoff = getenv("MMT_RING_COPY") == nullptr;   // tuning / A-B: copy launches instead
  HIPCHECK(e, hipHostGetDevicePointer((void**)&e->hring.params, e->params_host, 0));
  HIPCHECK(e, hipHostGetDevicePointer((void**)&e->hring.outs, e->outs_host, 0));
  for (auto& t : e->ring) HIPCHECK(e, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
  return MMT_OK;
}

// ---------------------------------------------------------------- timing probe
void probe_begin(mmt_engine* e, hipStream_t st, const char* cls, double flops, double bytes) {
  TimingProbe* p = e->probe.get();
  if (!p || p->cls != cls) return;
  if (p->capture) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    p->capture->ev.push_back({a, b});
    p->capture->work.push_back({flops, bytes});
    hipEventRecord(a, st);
    return;
  }
  if (p->used == p->ev.size()) {
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    p->ev.push_back({a, b});
  }
  hipEventRecord(p->ev[p->used].first, st);
  p->pending_work.push_back({flops, bytes});
}
void probe_end(mmt_engine* e, hipStream_t st, const char* cls) {
  TimingProbe* p = e->probe.get();
  if (!p || p->cls != cls) return;
  if (p->capture) {
    hipEventRecord(p->capture->ev.back().second, st);
    return;
  }
  hipEventRecord(p->ev[p->used].second, st);
  p->used++;
}
void probe_collect_graph(mmt_engine* e, const GraphEntry& g) {
  TimingProbe* p = e->probe.get();
  if (!p) return;
  for (size_t i = 0; i < g.ev.size(); ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, g.ev[i].first, g.ev[i].second) == hipSuccess) {
      p->total_ms += ms;
      p->launches++;
      p->flops += g.work[i].first;
      p->bytes += g.work[i].second;
    }
  }
}

void probe_collect(mmt_engine* e) {
  TimingProbe* p = e->probe.get();
  if (!p) return;
  for (size_t i = 0; i < p->used; ++i) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p->ev[i].first, p->ev[i].second) == hipSuccess) {
      p->total_ms += ms;
      p->launches++;
      p->flops += p->pending_work[i].first;
      p->bytes += p->pending_work[i].second;
    }
  }
  p->used = 0;
  p->pending_work.clear();
}

// ---------------------------------------------------------------- the per-frame launch sequence
GemmArgs dense(mmt_engine* e, float* ws, const bf16_t* A, const bf16_t* Al, int64_t lda, const bf16_t* W,
               const bf16_t* Wl, int64_t ldw, const float* bias, void* Cp, void* Cl, int64_t ldc, const float* R,
               int64_t ldr, int M, int N, int K) {
  GemmArgs a{};
  a.g[0] = GemmGroup{A, Al, lda, W, Wl, ldw, bias, Cp, Cl, ldc, R, ldr};
  a.groups = 1;
  a.split = e->split ? 1 : 0;
  a.zero = e->zero;
  a.M = M;
  a.N = N;
  a.K = K;
  a.amode = A_DENSE;
  // GEMMs with few 64 x 64 tiles and a long K (small batches: fc2 / proj / head convs at one or two
  // sequences) split K over workgroups into this stream half's workspace, reduced in a fixed order with the
  // epilogue (gemm.hip).  The summation order then depends on the batch size: results agree across batch
  // sizes to fp32 rounding, not bit for bit (test_batch_equals_single).
  a.ws = ws;
  a.ws_elems = ws ? kSplitKWsElems : 0;
  a.conc = e->conc_parts;
  return a;
}

// f16x3 scaling of a GEMM's groups: acc * 1 / (s_A s_W), 16-bit outputs split at out_scale
GemmArgs scaled(GemmArgs a, float sa_sw, float out_scale) {
  for (int k = 0; k < 3; ++k) {
    a.g[k].inv = 1.0f / sa_sw;
    a.g[k].out_scale = out_scale;
  }
  return a;
}

// returns gemm()'s K splits (> 1 only with a.defer_reduce: the partial slabs are left in a.ws); where no kernel
// runs this GEMM nothing is launched: -1, ok = false and the reason in e->err
int run_gemm(mmt_engine* e, bool& ok, hipStream_t st, const char* cls, const GemmArgs& a, int epi) {
  const double flops = 2.0 * a.M * a.N * (double)a.K * a.groups;
  // algorithmic HBM bytes: A and W once, C once (bf16 or fp32), R once for the residual epilogues
  const bool out16 = epi == EPI_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RELU_BF16;
  const double outb = (double)a.M * a.N * (out16 ? 2.0 : 4.0) * (a.split && out16 ? 2.0 : 1.0);
  const double rb = (epi == EPI_RESID_F32) ? (double)a.M * a.N * 4.0 : 0.0;
  const double bytes = (((double)a.M * a.K + (double)a.N * a.K) * 2.0 * (a.split ? 2.0 : 1.0) + outb + rb) * a.groups;
  probe_begin(e, st, cls, flops, bytes);
  const char* why = nullptr;
  const int ks = gemm(a, epi, st, &why);
  probe_end(e, st, cls);
  if (ks < 0) {
    e->err = std::string("gemm ") + cls + ": " + why;
    ok = false;
  }
  return ks;
}

// a token kernel's launcher declined (more than 1 024 search tokens / slots per sequence): nothing was launched
void token_fail(mmt_engine* e, bool& ok, const char* what) {
  e->err = std::string(what) + ": more than 1024 tokens per sequence";
  ok = false;
}

// a residual-stream GEMM (EPI_RESID_F32 into X) whose split-K combine is left to the consuming row kernel
RowReduce run_resid_gemm(mmt_engine* e, bool& ok, hipStream_t st, const char* cls, GemmArgs a) {
  a.defer_reduce = a.ws ? 1 : 0;
  const int ks = run_gemm(e, ok, st, cls, a, EPI_RESID_F32);
  RowReduce rr{};
  if (ks > 1) rr = RowReduce{a.ws, ks, (int64_t)a.M * a.N, a.g[0].inv, a.g[0].bias};
  return rr;
}

// offset a possibly-null low-half pointer
template <class T>
inline T* off(T* p, size_t o) {
  return p ? p + o : nullptr;
}

// false: a GEMM of the launch has no kernel (e->err says which); the rest was enqueued all the same
bool enqueue_forward(mmt_engine* e, int b0, int r0, int n, hipStream_t s, int part, bool fuse_geom) {
  bool ok = true;
  const auto& c = e->cfg;
  const int Lz = e->Lz, Lx = e->Lx, L = e->L;
  // per-launch activation views: this launch covers launch-relative sequences [r0, r0 + n)
  // split-K workspace per stream half; parity mode only (in bf16 a different summation order can flip a
  // bf16 rounding and, through CE, a box: that mode keeps batch-size-independent results instead)
  float* const q_ws = e->split ? e->splitk_ws + (size_t)part * kSplitKWsElems : nullptr;
  auto* const q_X = off(e->X, (size_t)r0 * (size_t)L * C);
  auto* const q_X2 = off(e->X2, (size_t)r0 * (size_t)L * C);
  auto* const q_tok_rgb = off(e->tok_rgb, (size_t)r0 * (size_t)L * C);
  auto* const q_tok_aux = off(e->tok_aux, (size_t)r0 * (size_t)L * C);
  const size_t a8half = (size_t)c.max_batch * L * 8;   // layer i's a8 / c8 live in half i & 1
  auto q_a8 = [&](int i) { return e->a8 + (size_t)(i & 1) * a8half + (size_t)r0 * L * 8; };
  auto q_c8 = [&](int i) { return e->c8 + (size_t)(i & 1) * a8half + (size_t)r0 * L * 8; };
  auto* const q_Hn = off(e->Hn, (size_t)r0 * (size_t)L * C);
  auto* const q_Hn_l = off(e->Hn_l, (size_t)r0 * (size_t)L * C);
  auto* const q_QKV = off(e->QKV, (size_t)r0 * (size_t)L * 3 * C);
  auto* const q_QKV_l = off(e->QKV_l, (size_t)r0 * (size_t)L * 3 * C);
  auto* const q_O = off(e->O, (size_t)r0 * (size_t)L * C);
  auto* const q_O_l = off(e->O_l, (size_t)r0 * (size_t)L * C);
  auto* const q_Hm = off(e->Hm, (size_t)r0 * (size_t)L * MLPD);
  auto* const q_Hm_l = off(e->Hm_l, (size_t)r0 * (size_t)L * MLPD);
  auto* const q_ce_prob = off(e->ce_prob, (size_t)r0 * (size_t)HEADS * Lx);
  auto* const q_feat = off(e->feat, (size_t)r0 * (size_t)Lx * C);
  auto* const q_feat_l = off(e->feat_l, (size_t)r0 * (size_t)Lx * C);
  auto* const q_dbg_feat = off(e->dbg_feat, (size_t)r0 * (size_t)L * C);
  auto* const q_h1 = off(e->h1, (size_t)r0 * (size_t)Lx * 3 * c.head_channels);
  auto* const q_h1_l = off(e->h1_l, (size_t)r0 * (size_t)Lx * 3 * c.head_channels);
  auto* const q_h2 = off(e->h2, (size_t)r0 * (size_t)Lx * 3 * (c.head_channels / 2));
  auto* const q_h2_l = off(e->h2_l, (size_t)r0 * (size_t)Lx * 3 * (c.head_channels / 2));
  auto* const q_h3 = off(e->h3, (size_t)r0 * (size_t)Lx * 3 * (c.head_channels / 4));
  auto* const q_h3_l = off(e->h3_l, (size_t)r0 * (size_t)Lx * 3 * (c.head_channels / 4));
  auto* const q_h4 = off(e->h4, (size_t)r0 * (size_t)Lx * 3 * 32);
  auto* const q_res = off(e->res, (size_t)r0 * (size_t)8);
  auto* const q_dbg_maps = off(e->dbg_maps, (size_t)r0 * (size_t)5 * Lx);
  auto* const q_gidx0 = off(e->gidx0, (size_t)r0 * (size_t)Lx);
  auto* const q_gidx1 = off(e->gidx1, (size_t)r0 * (size_t)Lx);
  auto* const q_slot2pos = off(e->slot2pos, (size_t)r0 * (size_t)Lx);
  auto* const q_gather = off(e->gather, (size_t)r0 * (size_t)L);
  auto* const q_removed = off(e->removed, (size_t)r0 * (size_t)Lx);
  auto* const q_dbg_patch = off(e->dbg_patch, (size_t)r0 * (size_t)c.search_size * c.search_size * c.in_chans);
  const bool vipt = c.model == MMT_MODEL_VIPT;
  const bool prompted = vipt && c.prompt_type != MMT_PROMPT_NONE;
  const bool deep = vipt && c.prompt_type == MMT_PROMPT_DEEP;
  bf16_t* A_rgb = e->A_rgb + (size_t)b0 * L * C;
  bf16_t* A_aux = e->A_aux + (size_t)b0 * L * C;
  bf16_t* A_rgb_l = off(e->A_rgb_l, (size_t)b0 * L * C);
  bf16_t* A_aux_l = off(e->A_aux_l, (size_t)b0 * L * C);

  // 1. (crop geometry: enqueue_split, once per launch) crop + normalise + patchify
  CropArgs ca{};
  ca.params = e->params_dev + r0;
  ca.B = n;
  ca.out_sz = c.search_size;
  ca.C = c.in_chans;
  ca.A_rgb = A_rgb;
  ca.A_aux = A_aux;
  ca.A_rgb_lo = A_rgb_l;
  ca.A_aux_lo = A_aux_l;
  ca.rows_per_seq = L;
  ca.row0 = Lz;
  ca.dbg_patch = q_dbg_patch;
  if (fuse_geom) {   // a launch not split into stream parts: the geometry kernel's work done by the crop itself
    ca.geom.state = e->state_dev + b0;
    ca.geom.factor = c.search_factor;
    ca.geom.ring = e->hring;
    ca.geom.use_ring = e->ring_handoff ? 1 : 0;
    ca.geom.gidx = q_gidx0;
    ca.geom.slot2pos = q_slot2pos;
    ca.geom.Lz = Lz;
    ca.geom.Lx = Lx;
  }
  crop_patchify(ca, s);

  // 2. patch embedding (template rows were written at initialize)
  float* X = q_X;
  float* X2 = q_X2;
  if (vipt) {
    GemmArgs g = dense(e, q_ws, A_rgb, A_rgb_l, C, e->pe_w, e->pe_wl, C, e->pe_b, q_tok_rgb, nullptr, C, nullptr, 0,
                       n * L, C, C);
    g.g[1] = GemmGroup{A_aux, A_aux_l, C, e->pep_w, e->pep_wl, C, e->pep_b, q_tok_aux, nullptr, C, nullptr, 0};
    g.groups = 2;
    g = scaled(g, kPixScale * e->pe_s, 1.0f);
    g.g[1].inv = 1.0f / (kPixScale * e->pep_s);
    run_gemm(e, ok, s, "patch", g, EPI_F32);
  } else {
    GemmArgs g = dense(e, q_ws, A_rgb, A_rgb_l, C, e->pe_w, e->pe_wl, C, e->pe_b, X, nullptr, C, e->pos, C, n * L, C, C);
    g.pos_rows = L;
    run_gemm(e, ok, s, "patch", scaled(g, kPixScale * e->pe_s, 1.0f), EPI_POS_F32);
  }
  // (the token index arrays gidx0 / slot2pos were reset by the launch's geometry kernel, enqueue_split)

  PromptArgs pa{};
  pa.B = n;
  pa.Lz = Lz;
  pa.Lx = Lx;
  auto set_prompt = [&](int i, int lnA) {
    pa.layer = i;
    pa.a8 = q_a8(i);
    pa.c8 = q_c8(i);
    pa.a8p = i ? q_a8(i - 1) : nullptr;
    pa.c8p = i ? q_c8(i - 1) : nullptr;
    pa.smooth_p = i ? e->pw[i - 1].smooth : 0.f;
    pa.fstat_p = i ? e->fstat + (size_t)r0 * 32 : nullptr;   // written by layer i-1's LN1 (prompt_expand_ln)
    pa.lnA_w = e->pw[lnA].nw;
    pa.lnA_b = e->pw[lnA].nb;
    pa.lnB_w = e->pw[i].nw;
    pa.lnB_b = e->pw[i].nb;
    pa.w00 = i ? e->pw[i].w00f : e->pw[i].w00;   // deep layers: LN_A's affine folded in
    pa.b00 = i ? e->pw[i].b00f : e->pw[i].b00;
    pa.w01 = e->pw[i].w01;
    pa.b01 = e->pw[i].b01;
    pa.fold = e->pw[i].fold;
    pa.smooth = e->pw[i].smooth;
  };
  if (prompted) {  // layer-0 prompt: vit_ce_prompt.py:205-219
    set_prompt(0, 0);
    pa.srcA = q_tok_rgb;
    pa.srcA_rows = L;
    pa.srcB = q_tok_aux;
    pa.slot2pos = nullptr;
    // fovea, P and X = tok_rgb + P + pos are formed with block 0's LN1
    if (!prompt_reduce(pa, s)) token_fail(e, ok, "prompt_reduce");
  }

  int* gin = q_gidx0;
  int* gout = q_gidx1;
  int removed_off = 0;
  int Ls = Lx;
  int ce_stage = 0;
  // a split-K update of the residual stream X still in the workspace (proj / fc2 of few-tile launches): the next
  // row kernel that reads X applies it and writes X back, instead of a reduce launch
  RowReduce pend{};
  for (int i = 0; i < DEPTH; ++i) {
    const LayerW& w = e->lw[i];
    const int Na = Lz + Ls;
    int ln_mode = (prompted && i == 0) ? 1 : 0;
    if (deep && i >= 1) {  // vit_ce_prompt.py:268-310
      set_prompt(i, i - 1);
      pa.srcA = X;
      pa.srcA_rows = Na;
      pa.srcB = nullptr;
      pa.slot2pos = q_slot2pos;
      pa.rr = pend;   // the previous block's fc2 update of X
      pend = RowReduce{};
      ln_mode = 2;    // prompt_reduce(pa) below, with LN1 or before it
    }
    if (ln_mode) {
      LnPromptArgs la{};
      la.mode = ln_mode;
      la.rows = n * Na;
      la.rows_per_seq = Na;
      la.Lz = Lz;
      la.Lx = Lx;
      la.X = X;
      la.a8 = q_a8(i);
      la.c8 = q_c8(i);
      la.smooth = e->pw[i].smooth;
      la.fstat = deep ? e->fstat + (size_t)r0 * 32 : nullptr;
      la.w1 = e->pw[i].w1;   // conv1x1 of the prompt block that ran for this layer
      la.b1 = e->pw[i].b1;
      la.tok_rgb = q_tok_rgb;
      la.pos = e->pos;
      la.gidx = gin;
      la.w = w.n1w;
      la.b = w.n1b;
      la.out = q_Hn;
      la.out_lo = q_Hn_l;
      la.out_scale = w.ln1_s;
      if (ln_mode == 2 && !prompt_reduce(pa, s)) token_fail(e, ok, "prompt_reduce");
      if (!prompt_expand_ln(la, s)) token_fail(e, ok, "prompt_expand_ln");
    } else {
      layernorm(X, w.n1w, w.n1b, q_Hn, q_Hn_l, w.ln1_s, nullptr, n * Na, Na, nullptr, Na, nullptr, s, pend);
      pend = RowReduce{};
    }
    run_gemm(e, ok, s, "qkv",
             scaled(dense(e, q_ws, q_Hn, q_Hn_l, C, w.qkv_w, w.qkv_wl, C, w.qkv_b, q_QKV, q_QKV_l, 3 * C, nullptr, 0,
                          n * Na, 3 * C, C),
                    w.ln1_s * w.qkv_s, w.qkv_os),
             EPI_BF16);
    const bool ce = e->keep_at[i] != e->ls_before[i];
    AttnArgs aa{};
    aa.qkv = q_QKV;
    aa.qkv_lo = q_QKV_l;
    aa.out = q_O;
    aa.out_lo = q_O_l;
    aa.qk_inv = 0.125f / (w.qkv_os * w.qkv_os);   // attn.py:15 scale 64^-0.5
    aa.pv_inv = 1.0f / (16384.0f * w.qkv_os);
    aa.out_scale = w.qkv_os;                      // |O| <= max |V|
    aa.B = n;
    aa.N = Na;
    aa.heads = HEADS;
    aa.ce_query = ce && !e->ce_mask ? c.ce_template_index : -1;
    aa.ce_lens_t = Lz;
    aa.ce_prob = q_ce_prob;
    // algorithmic bytes: Q, K, V in and O out, 2 B per element, twice in the parity mode (hi + lo planes: 12 288 B per
    // token row), as the GEMM classes count their operands
    probe_begin(e, s, "attn", 4.0 * n * HEADS * (double)Na * Na * 64, (double)n * Na * 4 * C * 2 * (e->split ? 2 : 1));
    attention(aa, s);
    probe_end(e, s, "attn");
    if (ce && e->ce_mask) {   // the mean over the slots' template masks instead of attention's single exported row
      CeRowsArgs cr{};
      cr.qkv = q_QKV;
      cr.qkv_lo = q_QKV_l;
      cr.B = n;
      cr.N = Na;
      cr.heads = HEADS;
      cr.lens_t = Lz;
      cr.rows = e->ce_rows + (size_t)b0 * Lz;
      cr.pitch = Lz;
      cr.nrows = e->ce_nrows + b0;
      cr.prob = q_ce_prob;
      cr.qk_inv = aa.qk_inv;
      // at most Lz rows against Na keys, twice (the search-key tiles are multiplied again): K of every head once
      probe_begin(e, s, "ce_rows", 2.0 * n * HEADS * (double)Lz * (2.0 * Na - Lz) * 64,
                  (double)n * Na * C * 2 * (e->split ? 2 : 1));
      ce_rows(cr, s);
      probe_end(e, s, "ce_rows");
    }
    pend = run_resid_gemm(
        e, ok, s, "proj",
        scaled(dense(e, q_ws, q_O, q_O_l, C, w.proj_w, w.proj_wl, C, w.proj_b, X, nullptr, C, X, C, n * Na, C, C),
               w.qkv_os * w.proj_s, 1.0f));
    if (ce) {  // attn_blocks.py:99-101
      const int keep = e->keep_at[i];
      CEArgs ce_a{};
      ce_a.B = n;
      ce_a.Lz = Lz;
      ce_a.Ls = Ls;
      ce_a.keep = keep;
      ce_a.heads = HEADS;
      ce_a.Lx = Lx;
      ce_a.prob = q_ce_prob;
      ce_a.gidx_in = gin;
      ce_a.gidx_out = gout;
      ce_a.gather = q_gather;
      ce_a.slot2pos = q_slot2pos;
      ce_a.removed = q_removed;
      ce_a.removed_off = removed_off;
      const size_t nce = std::max(c.n_ce, 1);
      ce_a.keys_pitch = (int)(nce * Lx);
      ce_a.keys_out = e->ce_keys ? e->ce_keys + (size_t)r0 * nce * Lx + (size_t)ce_stage * Lx : nullptr;
      ce_a.forced = (e->force_ce && e->ce_forced) ? e->ce_forced + (size_t)b0 * nce * Lx + (size_t)ce_stage * Lx
                                                  : nullptr;
      ++ce_stage;
      if (!ce_layernorm(ce_a, X, w.n2w, w.n2b, q_Hn, q_Hn_l, w.ln2_s, Na, X2, s, pend)) {
        if (!ce_select(ce_a, s)) token_fail(e, ok, "ce_select");
        layernorm(X, w.n2w, w.n2b, q_Hn, q_Hn_l, w.ln2_s, nullptr, n * (Lz + keep), Lz + keep, q_gather, Na, X2, s,
                  pend);
      }
      removed_off += Ls - keep;
      std::swap(gin, gout);
      Ls = keep;
      std::swap(X, X2);
    } else {
      layernorm(X, w.n2w, w.n2b, q_Hn, q_Hn_l, w.ln2_s, nullptr, n * Na, Na, nullptr, Na, nullptr, s, pend);
    }
    pend = RowReduce{};
    const int Nm = Lz + Ls;
    run_gemm(e, ok, s, "fc1",
             scaled(dense(e, q_ws, q_Hn, q_Hn_l, C, w.fc1_w, w.fc1_wl, C, w.fc1_b, q_Hm, q_Hm_l, MLPD, nullptr, 0,
                          n * Nm, MLPD, C),
                    w.ln2_s * w.fc1_s, w.fc1_os),
             EPI_GELU_BF16);
    pend = run_resid_gemm(e, ok, s, "fc2",
                          scaled(dense(e, q_ws, q_Hm, q_Hm_l, MLPD, w.fc2_w, w.fc2_wl, MLPD, w.fc2_b, X, nullptr, C, X, C,
                                       n * Nm, C, MLPD),
                                 w.fc1_os * w.fc2_s, 1.0f));
  }
  final_norm_recover(X, Lz + Ls, q_slot2pos, e->norm_w, e->norm_b, n, Lz, Lx, q_feat, q_feat_l, e->feat_s,
                     q_dbg_feat, s, pend);

  // CENTER head: conv1 of the three branches fused (N = 3*hc), then per-branch grouped convs
  const int hc = c.head_channels, fs = e->fs, M = n * Lx;
  {
    GemmArgs g = dense(e, q_ws, q_feat, q_feat_l, C, e->hw1, e->hw1l, 9 * C, e->hb1, q_h1, q_h1_l, 3 * hc, nullptr, 0,
                       M, 3 * hc, 9 * C);
    g.amode = A_CONV3;
    g.conv_hw = fs;
    g.conv_cin = C;
    run_gemm(e, ok, s, "conv1", scaled(g, e->feat_s * e->hw1_s, e->h_s[0]), EPI_RELU_BF16);
  }
  const int ch[4] = {hc, hc / 2, hc / 4, hc / 8};
  for (int j = 0; j < 3; ++j) {   // conv2, conv3, conv4
    const int ci = ch[j], co = ch[j + 1];
    GemmArgs g = dense(e, q_ws, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, M, co,
                       9 * ci);
    for (int k = 0; k < 3; ++k) {
      const bf16_t *A, *Al;
      int64_t lda;
      if (j == 0) {
        A = q_h1 + k * hc;
        Al = off(q_h1_l, (size_t)k * hc);
        lda = 3 * hc;
      } else {
        A = (j == 1 ? q_h2 : q_h3) + (size_t)k * M * ci;
        Al = off(j == 1 ? q_h2_l : q_h3_l, (size_t)k * M * ci);
        lda = ci;
      }
      void *Cout, *Cl;
      if (j == 0) {
        Cout = q_h2 + (size_t)k * M * co;
        Cl = off(q_h2_l, (size_t)k * M * co);
      } else if (j == 1) {
        Cout = q_h3 + (size_t)k * M * co;
        Cl = off(q_h3_l, (size_t)k * M * co);
      } else {
        Cout = q_h4 + (size_t)k * M * co;
        Cl = nullptr;
      }
      g.g[k] = GemmGroup{A, Al, lda, e->hw[j] + (size_t)k * co * 9 * ci, off(e->hwl[j], (size_t)k * co * 9 * ci),
                         9 * ci, e->hb[j] + k * co, Cout, Cl, co, nullptr, 0};
    }
    g.groups = 3;
    g.amode = A_CONV3;
    g.conv_hw = fs;
    g.conv_cin = ci;
    run_gemm(e, ok, s, j == 0 ? "conv2" : (j == 1 ? "conv3" : "conv4"),
             scaled(g, e->h_s[j] * e->hw_s[j], j < 2 ? e->h_s[j + 1] : 1.0f), j == 2 ? EPI_RELU_F32 : EPI_RELU_BF16);
  }
  DecodeArgs da{};
  da.B = n;
  da.fs = fs;
  da.h4 = q_h4;
  da.w5 = e->w5;
  da.b5 = e->b5;
  da.hann = e->hann;
  da.res = q_res;
  da.maps = q_dbg_maps;
  da.state = e->state_dev + b0;
  da.params = e->params_dev + r0;
  da.out = e->out_dev + r0;
  da.search_size = c.search_size;
  if (e->ring_handoff) {
    da.ring_outs = e->hring.outs;
    da.ring_cur = e->hring.cur;
    da.ring_pitch = e->hring.pitch;
    da.row0 = r0;
    if (fuse_geom) {
      da.ring_ctr = e->hring.ctr;
      da.ring_kring = e->hring.kring;
    }
  }
  decode(da, s);
  return ok;
}

// crop geometry of processing_utils.py:32-41 in doubles with Python rounding (round half to even)
int geometry(mmt_engine* e, const double box[4], double factor, int out_sz, int* x1, int* y1, int* crop_sz,
             double* rf) {
  const double x = box[0], y = box[1], w = box[2], h = box[3];
  const double cs = std::ceil(std::sqrt(w * h) * factor);
  if (!(cs >= 1.0)) return e->fail(MMT_E_BOX, "Too small bounding box.");
  if (cs > 1e6) return e->fail(MMT_E_ARG, "crop size out of range");
  *crop_sz = (int)cs;
  *x1 = (int)std::nearbyint(x + 0.5 * w - cs * 0.5);
  *y1 = (int)std::nearbyint(y + 0.5 * h - cs * 0.5);
  *rf = (double)out_sz / cs;
  return MMT_OK;
}

int stage_frame(mmt_engine* e, int slot, int ring, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t stride,
                int is_device, const uint8_t** dev, hipStream_t cs) {
  if (!frame || Hh < 2 || Ww < 2 || Cc != e->cfg.in_chans || stride < (int64_t)Ww * Cc)
    return e->fail(MMT_E_ARG, "bad frame (expect H x W x in_chans uint8, H,W >= 2)");
  if (is_device) {
    *dev = frame;
    return MMT_OK;
  }
  const size_t bytes = (size_t)stride * Hh;
  const size_t k = (size_t)slot * kRing + ring;
  if (e->frame_cap[k] < bytes) {
    if (e->frame_dev[k]) {
      HIPCHECK(e, hipStreamSynchronize(e->stream));
      HIPCHECK(e, hipStreamSynchronize(cs));
      hipFree(e->frame_dev[k]);
    }
    e->frame_dev[k] = nullptr;
    HIPCHECK(e, hipMalloc(&e->frame_dev[k], bytes));
    e->frame_cap[k] = bytes;
  }
  HIPCHECK(e, hipMemcpyAsync(e->frame_dev[k], frame, bytes, hipMemcpyHostToDevice, cs));
  *dev = e->frame_dev[k];
  return MMT_OK;
}

// One launch over n sequences.  Batches of >= overlap_min sequences run as two independent halves on
// two streams (fork/join events, also valid inside stream capture): the halves' kernels overlap, so one
// half's latency-bound kernels (LayerNorm, prompt, CE select, head tails) fill the CUs the other
// half's GEMM tails leave idle.  Each half owns disjoint activation rows, results are unchanged.
bool enqueue_split(mmt_engine* e, int b0, int n) {
  // crop geometry of all n sequences from their device-resident state (and, ring hand-off, their frame
  // parameters from the host ring), once per launch before any part starts
  if (e->overlap_min <= 0 || n < e->overlap_min || e->probe) {
    // one stream: the crop forms the geometry itself (MMT_GEOM_KERNEL, tuning: the separate geometry kernel)
    static const bool geom_kernel = getenv("MMT_GEOM_KERNEL") != nullptr;
    if (geom_kernel)
      crop_geometry(e->params_dev, e->state_dev + b0, n, e->cfg.search_factor, e->cfg.search_size,
                    e->ring_handoff ? &e->hring : nullptr, e->gidx0, e->slot2pos, e->Lz, e->Lx, e->stream);
    return enqueue_forward(e, b0, 0, n, e->stream, 0, !geom_kernel);
  }
  crop_geometry(e->params_dev, e->state_dev + b0, n, e->cfg.search_factor, e->cfg.search_size,
                e->ring_handoff ? &e->hring : nullptr, e->gidx0, e->slot2pos, e->Lz, e->Lx, e->stream);
  const int P = std::min(e->nparts, n);
  e->conc_parts = P;
  bool ok = true;
  hipEventRecord(e->fork_ev, e->stream);
  for (int p = 1; p < P; ++p) hipStreamWaitEvent(e->xstream[p - 1], e->fork_ev, 0);
  for (int p = 0; p < P; ++p) {
    const int r0 = n * p / P, r1 = n * (p + 1) / P;
    ok &= enqueue_forward(e, b0 + r0, r0, r1 - r0, p ? e->xstream[p - 1] : e->stream, p, false);
  }
  e->conc_parts = 1;
  for (int p = 1; p < P; ++p) {
    hipEventRecord(e->join_ev[p - 1], e->xstream[p - 1]);
    hipStreamWaitEvent(e->stream, e->join_ev[p - 1], 0);
  }
  return ok;
}

int launch(mmt_engine* e, int b0, int n, const GraphEntry** replayed) {
  *replayed = nullptr;
  // HIP does not time event-record nodes captured into a graph, so the kernel timing probe runs the
  // identical launch sequence eagerly, bracketing the probed kernel class with stream events
  if (!e->cfg.use_graphs || e->probe) {
    if (!enqueue_split(e, b0, n)) return MMT_E_ARG;
    ++e->launches;
    HIPCHECK(e, hipGetLastError());
    return MMT_OK;
  }
  const std::string pc = e->probe ? e->probe->cls : std::string();
  auto key = std::make_tuple(b0, n, pc);
  auto it = e->graphs.find(key);
  if (it == e->graphs.end()) {
    // first use of this batch shape: run eagerly (validates every launch, yields this frame's
    // result), then capture the identical launch sequence for replay
    TimingProbe* p = e->probe.get();
    if (p) {
      p->used = 0;
      p->pending_work.clear();
    }
    if (!enqueue_split(e, b0, n)) return MMT_E_ARG;
    ++e->launches;
    HIPCHECK(e, hipGetLastError());
    GraphEntry entry;
    if (p) p->capture = &entry;
    hipGraph_t g;
    hipError_t st = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    if (st == hipSuccess) {
      enqueue_split(e, b0, n);   // the same GEMMs as the eager pass above: it cannot fail here
      st = hipStreamEndCapture(e->stream, &g);
    }
    if (p) p->capture = nullptr;
    if (st != hipSuccess) return e->fail(MMT_E_HIP, std::string("graph capture: ") + hipGetErrorString(st));
    HIPCHECK(e, hipGraphInstantiate(&entry.exec, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    e->graphs.emplace(key, std::move(entry));
    return MMT_OK;
  }
  HIPCHECK(e, hipGraphLaunch(it->second.exec, e->stream));
  ++e->launches;
  *replayed = &it->second;
  return MMT_OK;
}

// the host copy of slot's state -> its device-resident copy (stream-ordered, synchronous)
int write_state(mmt_engine* e, int slot) {
  SeqState st{};
  for (int k = 0; k < 4; ++k) st.box[k] = e->state[slot][k];
  st.rf = 1.0;
  HIPCHECK(e, hipMemcpyAsync(e->state_dev + slot, &st, sizeof(SeqState), hipMemcpyHostToDevice, e->stream));
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  return MMT_OK;
}

int check_engine(mmt_engine* e) {
  if (!e) return MMT_E_ARG;
  if (!e->finalized) return e->fail(MMT_E_STATE, "engine not finalized (load every state_dict key first)");
  HIPCHECK(e, hipSetDevice(e->device));
  return MMT_OK;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

const char* mmt_version(void) { return "mmtrack-mi355x 0.1 (gfx950)"; }
int mmt_abi_version(void) { return MMT_ABI_VERSION; }
void* mmt_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return nullptr;
  return p;
}
void mmt_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int mmt_create(const mmt_config* cfg, int device, mmt_engine** out) {
  if (!cfg || !out) return MMT_E_ARG;
  *out = nullptr;
  auto e = std::make_unique<mmt_engine>();
  e->cfg = *cfg;
  e->device = device;
  const auto& c = e->cfg;
  if (c.template_size % 16 || c.search_size % 16 || c.template_size <= 0 || c.search_size <= 0 ||
      c.max_batch <= 0 || c.n_ce < 0 || c.n_ce > 12 || c.head_channels != 256 ||
      (c.model == MMT_MODEL_VIPT && (c.in_chans != 6 || c.prompt_type == MMT_PROMPT_NONE)) ||
      (c.model == MMT_MODEL_OSTRACK && c.in_chans != 3)) {
    *out = nullptr;
    return MMT_E_ARG;
  }
  e->Lz = (c.template_size / 16) * (c.template_size / 16);
  e->Lx = (c.search_size / 16) * (c.search_size / 16);
  e->L = e->Lz + e->Lx;
  e->fs = c.search_size / 16;
  e->tfs = c.template_size / 16;
  e->ce_mask = c.ce_template_index == MMT_CE_TEMPLATE_MASK;
  if (e->L > 1024 || (c.n_ce > 0 && !e->ce_mask && (c.ce_template_index < 0 || c.ce_template_index >= e->Lz)))
    return MMT_E_ARG;
  if (c.precision < 0 || c.precision > 1) return MMT_E_ARG;
  e->split = c.precision == 1;
  e->nprompt = c.model == MMT_MODEL_VIPT ? (c.prompt_type == MMT_PROMPT_DEEP ? DEPTH : (c.prompt_type ? 1 : 0)) : 0;
  int Ls = e->Lx;
  for (int i = 0; i < DEPTH; ++i) {
    e->ls_before.push_back(Ls);
    for (int k = 0; k < c.n_ce; ++k)
      if (c.ce_loc[k] == i) {
        const int keep = (int)std::ceil(c.ce_keep_ratio[k] * Ls);  // attn_blocks.py:40
        if (keep < Ls && keep > 0) Ls = keep;
      }
    e->keep_at.push_back(Ls);
  }
  if (hipSetDevice(device) != hipSuccess) return MMT_E_HIP;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  for (auto& xs : e->xstream)
    if (hipStreamCreateWithFlags(&xs, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  if (hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking) != hipSuccess) return MMT_E_HIP;
  for (auto& ev : e->copy_ev)
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  if (hipEventCreateWithFlags(&e->frame_ev, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  for (auto& je : e->join_ev)
    if (hipEventCreateWithFlags(&je, hipEventDisableTiming) != hipSuccess) return MMT_E_HIP;
  if (hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming) != hipSuccess)
    return MMT_E_HIP;
  // f16x3 GEMMs are 3x longer, so halves of 16 sequences still fill the chip and the two streams fill each
  // other's tile-quantisation tails (+8 % at 32 sequences; plain bf16 lost 4 % there)
  if (e->split) e->overlap_min = 32;
  if (const char* ov = std::getenv("MMT_OVERLAP_MIN")) e->overlap_min = std::atoi(ov);
  if (const char* np = std::getenv("MMT_NPARTS")) e->nparts = std::min(std::max(std::atoi(np), 2), mmt_engine::kMaxParts);
  build_expected(e.get());
  e->frame_dev.assign((size_t)c.max_batch * kRing, nullptr);
  e->frame_cap.assign((size_t)c.max_batch * kRing, 0);
  e->state.assign(c.max_batch, {0, 0, 0, 0});
  e->active.assign(c.max_batch, 0);
  if (alloc_acts(e.get()) != MMT_OK) return MMT_E_HIP;
  *out = e.release();
  return MMT_OK;
}

void mmt_destroy(mmt_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipStreamSynchronize(e->stream);
  for (auto& kv : e->graphs) {
    hipGraphExecDestroy(kv.second.exec);
    for (auto& pr : kv.second.ev) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  }
  if (e->probe)
    for (auto& p : e->probe->ev) {
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
  for (auto* p : e->frame_dev)
    if (p) hipFree(p);
  if (e->warena) hipFree(e->warena);
  if (e->aarena) hipFree(e->aarena);
  if (e->params_host) hipHostFree(e->params_host);
  if (e->outs_host) hipHostFree(e->outs_host);
  for (auto& t : e->ring)
    if (t.done) hipEventDestroy(t.done);
  if (e->stream) hipStreamDestroy(e->stream);
  for (auto& xs : e->xstream)
    if (xs) hipStreamDestroy(xs);
  if (e->cstream) {
    hipStreamSynchronize(e->cstream);
    hipStreamDestroy(e->cstream);
  }
  for (auto& ev : e->copy_ev)
    if (ev) hipEventDestroy(ev);
  if (e->frame_ev) hipEventDestroy(e->frame_ev);
  if (e->fork_ev) hipEventDestroy(e->fork_ev);
  for (auto& je : e->join_ev)
    if (je) hipEventDestroy(je);
  delete e;
}

const char* mmt_last_error(const mmt_engine* e) { return e ? e->err.c_str() : "null engine"; }

int mmt_num_expected_keys(const mmt_engine* e) { return e ? (int)e->expected_order.size() : 0; }
const char* mmt_expected_key(const mmt_engine* e, int i) {
  return (e && i >= 0 && i < (int)e->expected_order.size()) ? e->expected_order[i].c_str() : nullptr;
}

int mmt_set_tensor(mmt_engine* e, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!e || !key || (!data && ndim > 0)) return MMT_E_ARG;
  auto it = e->expected.find(key);
  if (it == e->expected.end()) return e->fail(MMT_E_WEIGHTS, std::string("Unexpected key(s) in state_dict: ") + key);
  std::vector<int64_t> shp(shape, shape + ndim);
  if (shp != it->second) return e->fail(MMT_E_WEIGHTS, std::string("size mismatch for ") + key);
  int64_t n = 1;
  for (auto d : shp) n *= d;
  HostTensor t;
  t.shape = shp;
  t.data.assign(data, data + (ndim ? n : 1));
  e->host[key] = std::move(t);
  e->finalized = false;
  return MMT_OK;
}

int mmt_finalize(mmt_engine* e) {
  if (!e) return MMT_E_ARG;
  std::string missing;
  for (auto& k : e->expected_order)
    if (!e->host.count(k)) missing += (missing.empty() ? "" : ", ") + k;
  if (!missing.empty()) return e->fail(MMT_E_WEIGHTS, "Missing key(s) in state_dict: " + missing);
  HIPCHECK(e, hipSetDevice(e->device));
  if (e->warena) {
    hipFree(e->warena);
    e->warena = nullptr;
    e->wused = 0;
  }
  for (auto& kv : e->graphs) {
    hipGraphExecDestroy(kv.second.exec);
    for (auto& pr : kv.second.ev) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  }
  e->graphs.clear();
  int r = pack_weights(e);
  if (r != MMT_OK) return r;
  e->host.clear();
  e->finalized = true;
  return MMT_OK;
}

// device frames are read in place: order the engine stream after the work queued so far on the
// caller's producer stream (e.g. the GPU frame assembly of mmt_rgbd_assemble / mmt_rgbx_merge)
static int wait_frame_stream(mmt_engine* e) {
  if (!e->frame_wait) return MMT_OK;
  // a caller stream with nothing left to run has already produced the frames: no event hop between the launches
  // (one sequence 1 124 -> 1 130 frames/s, 32 sequences level, profiles/r06_ab_frame_query.txt)
  if (hipStreamQuery(e->frame_stream) == hipSuccess) return MMT_OK;
  HIPCHECK(e, hipEventRecord(e->frame_ev, e->frame_stream));
  HIPCHECK(e, hipStreamWaitEvent(e->stream, e->frame_ev, 0));
  return MMT_OK;
}

int mmt_set_frame_stream(mmt_engine* e, void* hip_stream) {
  int r = check_engine(e);
  if (r) return r;
  e->frame_stream = (hipStream_t)hip_stream;
  e->frame_wait = true;
  return MMT_OK;
}

int mmt_initialize(mmt_engine* e, int slot, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride,
                   int is_device, const double init_xywh[4]) {
  int r = check_engine(e);
  if (r) return r;
  if (slot < 0 || slot >= e->cfg.max_batch || !init_xywh) return e->fail(MMT_E_ARG, "bad slot / box");
  if (e->unfetched) return e->fail(MMT_E_STATE, "initialize with unfetched frames in flight");
  int x1, y1, cs;
  double rf;
  TRY(geometry(e, init_xywh, e->cfg.template_factor, e->cfg.template_size, &x1, &y1, &cs, &rf));
  const uint8_t* dev;
  if (is_device) TRY(wait_frame_stream(e));
  TRY(stage_frame(e, slot, 0, frame, Hh, Ww, Cc, row_stride, is_device, &dev, e->stream));
  CropParam p{dev, row_stride, Hh, Ww, Cc, x1, y1, cs, 0};
  e->params_host[0] = p;
  HIPCHECK(e, hipMemcpyAsync(e->params_dev, e->params_host, sizeof(CropParam), hipMemcpyHostToDevice, e->stream));
  CropArgs ca{};
  ca.params = e->params_dev;
  ca.B = 1;
  ca.out_sz = e->cfg.template_size;
  ca.C = e->cfg.in_chans;
  ca.A_rgb = e->A_rgb + (size_t)slot * e->L * C;
  ca.A_aux = e->A_aux + (size_t)slot * e->L * C;
  ca.A_rgb_lo = off(e->A_rgb_l, (size_t)slot * e->L * C);
  ca.A_aux_lo = off(e->A_aux_l, (size_t)slot * e->L * C);
  ca.rows_per_seq = e->L;
  ca.row0 = 0;
  ca.dbg_patch = nullptr;
  crop_patchify(ca, e->stream);
  HIPCHECK(e, hipGetLastError());
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  e->state[slot] = {init_xywh[0], init_xywh[1], init_xywh[2], init_xywh[3]};
  TRY(write_state(e, slot));
  e->active[slot] = 1;
  return MMT_OK;
}

int mmt_track_batch_submit(mmt_engine* e, int first_slot, int n, const uint8_t* const* frames, const int* Hs,
                           const int* Ws, int Cc, const int64_t* row_stride, int is_device, int64_t* ticket) {
  int r = check_engine(e);
  if (r) return r;
  if (n <= 0 || first_slot < 0 || first_slot + n > e->cfg.max_batch || !frames || !Hs || !Ws || !row_stride ||
      !ticket)
    return e->fail(MMT_E_ARG, "bad batch");
  auto& t = e->ring[e->next_ticket % kRing];
  if (t.open) return e->fail(MMT_E_STATE, "too many unfetched frames (fetch before submitting more)");
  if (e->probe && e->unfetched > 0) return e->fail(MMT_E_STATE, "the timing probe needs fetch before the next submit");
  const int entry = (int)(e->launches % kRing);   // the ring entry this launch's geometry / decode use
  CropParam* ph = e->params_host + (size_t)entry * e->cfg.max_batch;
  for (int i = 0; i < n; ++i) {
    const int slot = first_slot + i;
    if (!e->active[slot]) return e->fail(MMT_E_STATE, "track() before initialize() on slot " + std::to_string(slot));
    // with nothing in flight the host copy of the state is current: reject a bad box before any work
    // (the reference raises before touching its state); in flight, the device flags it per frame
    if (e->unfetched == 0) {
      int x1, y1, cs;
      double rf;
      TRY(geometry(e, e->state[slot].data(), e->cfg.search_factor, e->cfg.search_size, &x1, &y1, &cs, &rf));
    }
    const uint8_t* dev;
    TRY(stage_frame(e, slot, (int)(e->next_ticket % kRing), frames[i], Hs[i], Ws[i], Cc, row_stride[i], is_device,
                    &dev, e->cstream));
    ph[i] = CropParam{dev, row_stride[i], Hs[i], Ws[i], Cc, 0, 0, 0, 0};   // geometry: crop_geometry()
  }
  if (is_device) TRY(wait_frame_stream(e));
  if (!is_device) {   // the launch waits for this frame's copies only (copy stream, overlapping compute)
    hipEvent_t ce = e->copy_ev[e->next_ticket % kRing];
    HIPCHECK(e, hipEventRecord(ce, e->cstream));
    HIPCHECK(e, hipStreamWaitEvent(e->stream, ce, 0));
  }
  if (!e->ring_handoff)
    HIPCHECK(e, hipMemcpyAsync(e->params_dev, ph, n * sizeof(CropParam), hipMemcpyHostToDevice, e->stream));
  const GraphEntry* replayed = nullptr;
  TRY(launch(e, first_slot, n, &replayed));
  if (!e->ring_handoff) {
    TrackOut* oh = e->outs_host + (size_t)entry * e->cfg.max_batch;
    HIPCHECK(e, hipMemcpyAsync(oh, e->out_dev, (size_t)n * sizeof(TrackOut), hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHECK(e, hipEventRecord(t.done, e->stream));
  t.id = e->next_ticket++;
  t.first = first_slot;
  t.n = n;
  t.open = true;
  t.replayed = replayed;
  t.entry = entry;
  ++e->unfetched;
  *ticket = t.id;
  e->last_batch = n;
  return MMT_OK;
}

int mmt_track_batch_fetch(mmt_engine* e, int64_t ticket, double* out_xywh, float* out_score) {
  if (!e) return MMT_E_ARG;
  if (ticket < 0) return e->fail(MMT_E_ARG, "bad ticket");
  auto& t = e->ring[ticket % kRing];
  if (!t.open || t.id != ticket) return e->fail(MMT_E_ARG, "unknown or already fetched ticket");
  HIPCHECK(e, hipSetDevice(e->device));
  HIPCHECK(e, hipEventSynchronize(t.done));
  t.open = false;
  --e->unfetched;
  if (t.replayed)
    probe_collect_graph(e, *t.replayed);
  else
    probe_collect(e);
  const TrackOut* oh = e->outs_host + (size_t)t.entry * e->cfg.max_batch;
  int rc = MMT_OK;
  for (int i = 0; i < t.n; ++i) {
    const int slot = t.first + i;
    e->state[slot] = {oh[i].box[0], oh[i].box[1], oh[i].box[2], oh[i].box[3]};
    if (out_xywh)
      for (int k = 0; k < 4; ++k) out_xywh[4 * i + k] = oh[i].box[k];
    if (out_score) out_score[i] = oh[i].score;
    if (oh[i].err && rc == MMT_OK)
      rc = e->fail(oh[i].err, oh[i].err == MMT_E_BOX ? "Too small bounding box." : "crop size out of range");
  }
  return rc;
}

int mmt_track_batch(mmt_engine* e, int first_slot, int n, const uint8_t* const* frames, const int* Hs,
                    const int* Ws, int Cc, const int64_t* row_stride, int is_device, double* out_xywh,
                    float* out_score) {
  int64_t ticket;
  int r = mmt_track_batch_submit(e, first_slot, n, frames, Hs, Ws, Cc, row_stride, is_device, &ticket);
  if (r) return r;
  return mmt_track_batch_fetch(e, ticket, out_xywh, out_score);
}

int mmt_track(mmt_engine* e, int slot, const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride,
              int is_device, double out_xywh[4], float* out_score) {
  return mmt_track_batch(e, slot, 1, &frame, &Hh, &Ww, Cc, &row_stride, is_device, out_xywh, out_score);
}

int mmt_get_state(const mmt_engine* e, int slot, double out_xywh[4]) {
  if (!e || slot < 0 || slot >= e->cfg.max_batch || !out_xywh) return MMT_E_ARG;
  for (int k = 0; k < 4; ++k) out_xywh[k] = e->state[slot][k];
  return MMT_OK;
}

int mmt_set_state(mmt_engine* e, int slot, const double xywh[4]) {
  if (!e || slot < 0 || slot >= e->cfg.max_batch || !xywh) return MMT_E_ARG;
  if (e->unfetched) return e->fail(MMT_E_STATE, "set_state with unfetched frames in flight");
  e->state[slot] = {xywh[0], xywh[1], xywh[2], xywh[3]};
  return write_state(e, slot);
}

int mmt_set_ce_template_mask(mmt_engine* e, int slot, const uint8_t* mask, int n) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->ce_mask) return e->fail(MMT_E_STATE, "engine not in mask mode (ce_template_index = MMT_CE_TEMPLATE_MASK)");
  if (!mask || n != e->Lz || slot < -1 || slot >= e->cfg.max_batch)
    return e->fail(MMT_E_ARG, "bad CE template mask (expect Lz bytes, slot in [-1, max_batch))");
  if (e->unfetched) return e->fail(MMT_E_STATE, "set_ce_template_mask with unfetched frames in flight");
  std::vector<int> rows(e->Lz, 0);
  int nr = 0;
  for (int i = 0; i < n; ++i)
    if (mask[i]) rows[nr++] = i;
  if (nr == 0) return e->fail(MMT_E_ARG, "CE template mask selects no token");
  // stream-ordered after the frames enqueued so far, synchronous (the host vectors die here), as write_state
  for (int sl = slot < 0 ? 0 : slot; sl < (slot < 0 ? e->cfg.max_batch : slot + 1); ++sl) {
    HIPCHECK(e, hipMemcpyAsync(e->ce_rows + (size_t)sl * e->Lz, rows.data(), (size_t)e->Lz * 4, hipMemcpyHostToDevice,
                               e->stream));
    HIPCHECK(e, hipMemcpyAsync(e->ce_nrows + sl, &nr, 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPCHECK(e, hipStreamSynchronize(e->stream));
  return MMT_OK;
}

int mmt_debug_fetch(mmt_engine* e, const char* what, int bi, void* dst, size_t nbytes) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->cfg.debug_outputs) return e->fail(MMT_E_STATE, "engine built without debug_outputs");
  if (!what || !dst || bi < 0 || bi >= e->cfg.max_batch) return e->fail(MMT_E_ARG, "bad debug fetch");
  const void* src = nullptr;
  size_t sz = 0;
  const std::string w(what);
  const int S = e->cfg.search_size;
  if (w == "crop") {
    sz = (size_t)S * S * e->cfg.in_chans;
    src = e->dbg_patch + bi * sz;
  } else if (w == "maps") {
    sz = (size_t)5 * e->Lx * 4;
    src = reinterpret_cast<const char*>(e->dbg_maps) + bi * sz;
  } else if (w == "feat") {
    sz = (size_t)e->L * C * 4;
    src = reinterpret_cast<const char*>(e->dbg_feat) + bi * sz;
  } else if (w == "removed") {
    sz = (size_t)e->Lx * 4;
    src = reinterpret_cast<const char*>(e->removed) + bi * sz;
  } else if (w == "result") {
    sz = 8 * 4;
    src = reinterpret_cast<const char*>(e->res) + bi * sz;
  } else if (w == "ce_keys") {
    sz = (size_t)std::max(e->cfg.n_ce, 1) * e->Lx * 4;
    src = reinterpret_cast<const char*>(e->ce_keys) + bi * sz;
  } else {
    return e->fail(MMT_E_ARG, "unknown debug buffer " + w);
  }
  if (nbytes < sz) return e->fail(MMT_E_ARG, "debug buffer too small");
  HIPCHECK(e, hipMemcpy(dst, src, sz, hipMemcpyDeviceToHost));
  return MMT_OK;
}

int mmt_debug_force_ce(mmt_engine* e, int slot, const float* keys, size_t n_floats) {
  int r = check_engine(e);
  if (r) return r;
  if (!e->cfg.debug_outputs) return e->fail(MMT_E_STATE, "engine built without debug_outputs");
  const size_t per = (size_t)std::max(e->cfg.n_ce, 1) * e->Lx;
  if (e->unfetched) return e->fail(MMT_E_STATE, "force_ce with unfetched frames in flight");
  if (!keys) {
    e->force_ce = false;
  } else {
    if (slot < 0 || slot >= e->cfg.max_batch || n_floats != per) return e->fail(MMT_E_ARG, "bad forced CE keys");
    HIPCHECK(e, hipMemcpy(e->ce_forced + (size_t)slot * per, keys, per * 4, hipMemcpyHostToDevice));
    e->force_ce = true;
  }
  // captured graphs carry the old kernel arguments
  for (auto& kv : e->graphs) {
    hipGraphExecDestroy(kv.second.exec);
    for (auto& pr : kv.second.ev) {
      hipEventDestroy(pr.first);
      hipEventDestroy(pr.second);
    }
  }
  e->graphs.clear();
  return MMT_OK;
}

int mmt_timing_enable(mmt_engine* e, const char* cls) {
  if (!e) return MMT_E_ARG;
  if (!cls || !*cls) {
    if (e->probe)
      for (auto& p : e->probe->ev) {
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
      }
    e->probe.reset();
    return MMT_OK;
  }
  if (!e->probe) e->probe = std::make_unique<TimingProbe>();
  e->probe->cls = cls;
  e->probe->launches = 0;
  e->probe->total_ms = e->probe->flops = e->probe->bytes = 0;
  return MMT_OK;
}

int mmt_timing_read(mmt_engine* e, int* launches, double* total_ms, double* flops, double* bytes) {
  if (!e || !e->probe) return MMT_E_STATE;
  if (launches) *launches = (int)e->probe->launches;
  if (total_ms) *total_ms = e->probe->total_ms;
  if (flops) *flops = e->probe->flops;
  if (bytes) *bytes = e->probe->bytes;
  return MMT_OK;
}

int mmt_xcorr(const float* z, const float* x, float* out, int B, int Cc, int hz, int wz, int hx, int wx, float scale,
              float bias, void* stream) {
  if (!z || !x || !out || B <= 0 || Cc <= 0 || hz <= 0 || wz <= 0 || hx < hz || wx < wz || 16 * hz * wz > 16384)
    return MMT_E_ARG;
  xcorr(z, x, out, B, Cc, hz, wz, hx, wx, scale, bias, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_xcorr_nhwc(const float* z, int64_t z_batch_stride, const float* x, float* out, int B, int Cc, int hz, int wz,
                   int hx, int wx, float scale, float bias, void* stream) {
  if (!z || !x || !out || B <= 0 || Cc <= 0 || hz <= 0 || wz <= 0 || hx < hz || wx < wz || z_batch_stride < 0 ||
      (int64_t)hz * wz * Cc > 16384 || ((Cc & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z) |
                                                           (uintptr_t)z_batch_stride * 4) & 15)))
    return MMT_E_ARG;
  xcorr_nhwc(z, z_batch_stride, x, out, B, Cc, hz, wz, hx, wx, scale, bias, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

static int siamfc_crop_impl(const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride, int n, const int* y0,
                            const int* x0, const int* size, const int pad[3], int out_sz, float* out, int nhwc,
                            void* stream) {
  if (!frame || !out || !y0 || !x0 || !size || !pad || n <= 0 || n > 8 || Hh <= 0 || Ww <= 0 || Cc < 3 ||
      row_stride < (int64_t)Ww * Cc || out_sz <= 0)
    return MMT_E_ARG;
  SiamCropArgs a{};
  a.frame = frame;
  a.stride = row_stride;
  a.H = Hh;
  a.W = Ww;
  a.C = Cc;
  a.n = n;
  a.out_sz = out_sz;
  for (int i = 0; i < n; ++i) {
    if (size[i] < 1) return MMT_E_ARG;
    a.y0[i] = y0[i];
    a.x0[i] = x0[i];
    a.size[i] = size[i];
  }
  for (int c = 0; c < 3; ++c) a.pad[c] = std::min(std::max(pad[c], 0), 255);
  a.out = out;
  a.nhwc = nhwc;
  siamfc_crop(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_siamfc_crop(const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride, int n, const int* y0,
                    const int* x0, const int* size, const int pad[3], int out_sz, float* out, void* stream) {
  return siamfc_crop_impl(frame, Hh, Ww, Cc, row_stride, n, y0, x0, size, pad, out_sz, out, 0, stream);
}

int mmt_siamfc_crop_nhwc(const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride, int n, const int* y0,
                         const int* x0, const int* size, const int pad[3], int out_sz, float* out, void* stream) {
  return siamfc_crop_impl(frame, Hh, Ww, Cc, row_stride, n, y0, x0, size, pad, out_sz, out, 1, stream);
}

int mmt_siamfc_response(const float* resp, int n, int r, int up, float scale_penalty, double window_influence,
                        const double* hann1d, double hann_sum, float* scratch, float* result, void* stream) {
  if (!resp || !hann1d || !scratch || !result || n <= 0 || n > 8 || r <= 1 || up < 2 || hann_sum <= 0)
    return MMT_E_ARG;
  SiamRespArgs a{};
  a.resp = resp;
  a.n = n;
  a.r = r;
  a.up = up;
  a.penalty = scale_penalty;
  a.one_minus_wi = (float)(1.0 - window_influence);
  a.wi = window_influence;
  a.hann_sum = hann_sum;
  a.hann1d = hann1d;
  a.scratch = scratch;
  a.result = result;
  siamfc_response(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* Cp, int64_t ldc,
                const float* R, int64_t ldr, int M, int N, int K, int epi, int conv_hw, int conv_cin, int pos_rows,
                void* stream) {
  if (!A || !W || !Cp || M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 32 || epi < 0 || epi > 6) return MMT_E_ARG;
  if ((epi == EPI_RESID_F32 || epi == EPI_POS_F32) && !R) return MMT_E_ARG;
  if (conv_hw > 0 && (conv_cin % 64 || K != 9 * conv_cin || (epi != EPI_RELU_BF16 && epi != EPI_RELU_F32)))
    return MMT_E_ARG;
  static bf16_t* zero = nullptr;
  static float* ws = nullptr;
  if (!zero && hipMalloc(&zero, 256) == hipSuccess) hipMemset(zero, 0, 256);
  if (!ws && hipMalloc(&ws, kSplitKWsElems * 4) != hipSuccess) ws = nullptr;
  if (ws) {   // the split-K workspace starts at zero
    static bool zeroed = hipMemset(ws, 0, kSplitKWsElems * 4) == hipSuccess;
    if (!zeroed) return MMT_E_HIP;
  }
  GemmArgs a{};
  a.g[0] = GemmGroup{(const bf16_t*)A, nullptr, lda, (const bf16_t*)W, nullptr, ldw, bias, Cp, nullptr, ldc, R, ldr};
  a.groups = 1;
  a.zero = zero;
  a.ws = ws;
  a.ws_elems = ws ? kSplitKWsElems : 0;
  a.M = M;
  a.N = N;
  a.K = K;
  a.amode = conv_hw > 0 ? A_CONV3 : A_DENSE;
  a.conv_hw = conv_hw;
  a.conv_cin = conv_cin;
  a.pos_rows = pos_rows > 0 ? pos_rows : 1;
  if (gemm(a, epi, (hipStream_t)stream) < 0) return MMT_E_ARG;   // no kernel for this shape / epilogue: nothing ran
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

// a split-K workspace of the engine's size for the operator entry points (zeroed once)
static float* op_workspace() {
  static float* ws = nullptr;
  if (!ws && hipMalloc(&ws, kSplitKWsElems * 4) == hipSuccess && hipMemset(ws, 0, kSplitKWsElems * 4) != hipSuccess) {
    hipFree(ws);
    ws = nullptr;
  }
  return ws;
}

int mmt_op_gemm_f16x3(const void* A_hi, const void* A_lo, int64_t lda, const void* W_hi, const void* W_lo, int64_t ldw,
                      const float* bias, void* C, void* C_lo, int64_t ldc, const float* R, int64_t ldr, int M, int N, int K,
                      int epi, float inv, float out_scale, int conv_hw, int conv_cin, void* stream) {
  if (!A_hi || !A_lo || !W_hi || !W_lo || !C || M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 32 || epi < 0 || epi > 6)
    return MMT_E_ARG;
  const bool out16 = epi == EPI_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RELU_BF16;
  if (out16 && !C_lo) return MMT_E_ARG;
  if ((epi == EPI_RESID_F32 || epi == EPI_POS_F32) && !R) return MMT_E_ARG;
  if (conv_hw > 0 && (conv_cin % 64 || K != 9 * conv_cin || (epi != EPI_RELU_BF16 && epi != EPI_RELU_F32)))
    return MMT_E_ARG;
  float* ws = op_workspace();
  GemmArgs a{};
  a.g[0] = GemmGroup{(const bf16_t*)A_hi, (const bf16_t*)A_lo, lda, (const bf16_t*)W_hi, (const bf16_t*)W_lo, ldw,
                     bias, C, out16 ? C_lo : nullptr, ldc, R, ldr, inv, out_scale};
  a.groups = 1;
  a.split = 1;
  a.ws = ws;
  a.ws_elems = ws ? kSplitKWsElems : 0;
  a.M = M;
  a.N = N;
  a.K = K;
  a.amode = conv_hw > 0 ? A_CONV3 : A_DENSE;
  a.conv_hw = conv_hw;
  a.conv_cin = conv_cin;
  a.pos_rows = 1;
  if (gemm(a, epi, (hipStream_t)stream) < 0) return MMT_E_ARG;   // no kernel for this shape / epilogue: nothing ran
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_attention_f16x3(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, int B, int N, int heads,
                           int ce_query, int ce_lens_t, float* ce_prob, float s_qkv, void* stream) {
  if (!qkv_hi || !qkv_lo || !out_hi || !out_lo || B <= 0 || N <= 0 || N > 1024 || heads <= 0 || !(s_qkv > 0))
    return MMT_E_ARG;
  if (ce_query >= 0 && (!ce_prob || ce_lens_t < 0 || ce_lens_t >= N || ce_query >= N)) return MMT_E_ARG;
  AttnArgs a{};
  a.qkv = (const bf16_t*)qkv_hi;
  a.qkv_lo = (const bf16_t*)qkv_lo;
  a.out = (bf16_t*)out_hi;
  a.out_lo = (bf16_t*)out_lo;
  a.B = B;
  a.N = N;
  a.heads = heads;
  a.ce_query = ce_query;
  a.ce_lens_t = ce_lens_t;
  a.ce_prob = ce_prob;
  a.qk_inv = 0.125f / (s_qkv * s_qkv);   // the engine's arguments (enqueue_forward), head dim 64
  a.pv_inv = 1.0f / (16384.0f * s_qkv);
  a.out_scale = s_qkv;
  attention(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

namespace {
// the lists of an operator-level ce_rows call, read back and checked (tests and composing hosts: synchronous)
int check_ce_rows(int B, int N, int heads, int lens_t, const int* rows, int pitch, const int* nrows, const float* prob) {
  if (B <= 0 || N <= 0 || N > 1024 || heads <= 0 || lens_t <= 0 || lens_t >= N || !rows || !nrows || !prob || pitch <= 0)
    return MMT_E_ARG;
  std::vector<int> hn(B), hr((size_t)B * pitch);
  if (hipMemcpy(hn.data(), nrows, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hr.data(), rows, hr.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return MMT_E_HIP;
  for (int b = 0; b < B; ++b) {
    if (hn[b] < 1 || hn[b] > lens_t || hn[b] > pitch) return MMT_E_ARG;
    for (int i = 0; i < hn[b]; ++i) {
      const int r = hr[(size_t)b * pitch + i];
      if (r < 0 || r >= lens_t || (i > 0 && r <= hr[(size_t)b * pitch + i - 1])) return MMT_E_ARG;
    }
  }
  return MMT_OK;
}
}  // namespace

int mmt_op_ce_rows_f16x3(const void* qkv_hi, const void* qkv_lo, int B, int N, int heads, int lens_t, const int* rows,
                         int rows_pitch, const int* nrows, float* ce_prob, float s_qkv, void* stream) {
  if (!qkv_hi || !qkv_lo || !(s_qkv > 0)) return MMT_E_ARG;
  const int r = check_ce_rows(B, N, heads, lens_t, rows, rows_pitch, nrows, ce_prob);
  if (r) return r;
  CeRowsArgs a{};
  a.qkv = (const bf16_t*)qkv_hi;
  a.qkv_lo = (const bf16_t*)qkv_lo;
  a.B = B;
  a.N = N;
  a.heads = heads;
  a.lens_t = lens_t;
  a.rows = rows;
  a.pitch = rows_pitch;
  a.nrows = nrows;
  a.prob = ce_prob;
  a.qk_inv = 0.125f / (s_qkv * s_qkv);   // mmt_op_attention_f16x3's
  ce_rows(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_ce_rows(const void* qkv, int B, int N, int heads, int lens_t, const int* rows, int rows_pitch,
                   const int* nrows, float* ce_prob, void* stream) {
  if (!qkv) return MMT_E_ARG;
  const int r = check_ce_rows(B, N, heads, lens_t, rows, rows_pitch, nrows, ce_prob);
  if (r) return r;
  CeRowsArgs a{};
  a.qkv = (const bf16_t*)qkv;
  a.qkv_lo = nullptr;
  a.B = B;
  a.N = N;
  a.heads = heads;
  a.lens_t = lens_t;
  a.rows = rows;
  a.pitch = rows_pitch;
  a.nrows = nrows;
  a.prob = ce_prob;
  ce_rows(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_gemm_stamps(void* dev_buf) { return gemm_set_stamps(dev_buf) == 0 ? MMT_OK : MMT_E_HIP; }

int mmt_gemm_force_config(int cfg) {
  gemm_force_config(cfg);
  return MMT_OK;
}

int mmt_op_attention(const void* qkv, void* out, int B, int N, int heads, int ce_query, int ce_lens_t,
                     float* ce_prob, void* stream) {
  if (!qkv || !out || B <= 0 || N <= 0 || N > 1024 || heads <= 0) return MMT_E_ARG;
  if (ce_query >= 0 && (!ce_prob || ce_lens_t < 0 || ce_lens_t >= N || ce_query >= N)) return MMT_E_ARG;
  AttnArgs a{};
  a.qkv = (const bf16_t*)qkv;
  a.qkv_lo = nullptr;
  a.out = (bf16_t*)out;
  a.out_lo = nullptr;
  a.B = B;
  a.N = N;
  a.heads = heads;
  a.ce_query = ce_query;
  a.ce_lens_t = ce_lens_t;
  a.ce_prob = ce_prob;
  attention(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_layernorm(const float* x, const float* w, const float* b, void* out_bf16, float* out_f32, int rows,
                     void* stream) {
  if (!x || !w || !b || rows <= 0 || (!out_bf16 && !out_f32)) return MMT_E_ARG;
  layernorm(x, w, b, (bf16_t*)out_bf16, nullptr, 1.0f, out_f32, rows, rows, nullptr, rows, nullptr,
            (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

// ---- token kernels (tokens.hip)
namespace {
// a RowReduce from the C struct (null: nothing pending); false: bad fields
bool to_row_reduce(const mmt_row_reduce* r, RowReduce& rr) {
  rr = RowReduce{};
  if (!r || !r->ws) return true;
  if (r->ks < 1 || r->ks > 8 || r->slab < 0 || !r->bias) return false;
  rr = RowReduce{r->ws, r->ks, r->slab, r->inv, r->bias};
  return true;
}
// an index list of an operator-level call, read back and checked against [lo, hi) (tests and composing hosts:
// synchronous)
int check_index_list(const int* dev, size_t n, int lo, int hi) {
  std::vector<int> h(n);
  if (hipMemcpy(h.data(), dev, n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return MMT_E_HIP;
  for (int v : h)
    if (v < lo || v >= hi) return MMT_E_ARG;
  return MMT_OK;
}
}  // namespace

int mmt_tokens_force_config(int rows_per_wave, int rows_per_block) {
  return tokens_force_config(rows_per_wave, rows_per_block) ? MMT_OK : MMT_E_ARG;
}

int mmt_op_layernorm_ex(const float* x, const float* w, const float* b, void* out, void* out_lo, float out_scale,
                        float* out_f32, int rows, int rows_per_seq, const int* gather, int in_rows_per_seq,
                        float* xcopy, const mmt_row_reduce* reduce, void* stream) {
  RowReduce rr;
  if (!x || !w || !b || rows <= 0 || rows_per_seq <= 0 || rows % rows_per_seq || (!out && !out_f32 && !xcopy) ||
      (out_lo && !out) || !to_row_reduce(reduce, rr))
    return MMT_E_ARG;
  if (gather) {
    if (in_rows_per_seq <= 0) return MMT_E_ARG;
    const int r = check_index_list(gather, (size_t)rows, 0, in_rows_per_seq);
    if (r) return r;
  }
  layernorm(x, w, b, (bf16_t*)out, (bf16_t*)out_lo, out_scale, out_f32, rows, rows_per_seq, gather, in_rows_per_seq,
            xcopy, (hipStream_t)stream, rr);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_ce_select(const mmt_ce_args* c, int fused, const float* x, const float* w, const float* b, void* out,
                     void* out_lo, float out_scale, int in_rows_per_seq, float* xcopy, const mmt_row_reduce* reduce,
                     void* stream) {
  RowReduce rr;
  if (!c || c->B < 1 || c->Lz < 0 || c->Ls < 1 || c->Ls > 1024 || c->keep < 1 || c->keep > c->Ls || c->heads < 1 ||
      c->Lx < c->Ls || c->removed_off < 0 || c->removed_off + (c->Ls - c->keep) > c->Lx || !c->prob || !c->gidx_in ||
      !c->gidx_out || !c->gather || !c->slot2pos || !c->removed)
    return MMT_E_ARG;
  if (fused < 0 || fused > 1 || !x || !w || !b || (!out && !xcopy) || (out_lo && !out) ||
      in_rows_per_seq < c->Lz + c->Ls || !to_row_reduce(reduce, rr))
    return MMT_E_ARG;
  const int r = check_index_list(c->gidx_in, (size_t)c->B * c->Ls, 0, c->Lx);
  if (r) return r;
  CEArgs a{};
  a.B = c->B;
  a.Lz = c->Lz;
  a.Ls = c->Ls;
  a.keep = c->keep;
  a.heads = c->heads;
  a.Lx = c->Lx;
  a.prob = c->prob;
  a.gidx_in = c->gidx_in;
  a.gidx_out = c->gidx_out;
  a.gather = c->gather;
  a.slot2pos = c->slot2pos;
  a.removed = c->removed;
  a.removed_off = c->removed_off;
  const hipStream_t s = (hipStream_t)stream;
  if (fused) {   // the one-launch form or nothing: a caller asking for it is not handed the two-launch result
    if (!ce_layernorm(a, x, w, b, (bf16_t*)out, (bf16_t*)out_lo, out_scale, in_rows_per_seq, xcopy, s, rr))
      return MMT_E_STATE;
  } else {       // the engine's two-launch branch (enqueue_forward)
    if (!ce_select(a, s)) return MMT_E_ARG;
    layernorm(x, w, b, (bf16_t*)out, (bf16_t*)out_lo, out_scale, nullptr, c->B * (c->Lz + c->keep), c->Lz + c->keep,
              c->gather, in_rows_per_seq, xcopy, s, rr);
  }
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_final_norm_recover(const float* X, int rows_per_seq, const int* slot2pos, const float* w, const float* b,
                              int B, int Lz, int Lx, void* feat, void* feat_lo, float feat_scale, float* feat_f32,
                              const mmt_row_reduce* reduce, void* stream) {
  RowReduce rr;
  if (!X || !slot2pos || !w || !b || !feat || B < 1 || Lz < 0 || Lx < 1 || rows_per_seq < Lz || rows_per_seq < 1 ||
      !to_row_reduce(reduce, rr))
    return MMT_E_ARG;
  const int r = check_index_list(slot2pos, (size_t)B * Lx, -1, rows_per_seq);
  if (r) return r;
  final_norm_recover(X, rows_per_seq, slot2pos, w, b, B, Lz, Lx, (bf16_t*)feat, (bf16_t*)feat_lo, feat_scale, feat_f32,
                     (hipStream_t)stream, rr);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_prompt_reduce(const mmt_prompt_args* p, const mmt_row_reduce* reduce, void* stream) {
  RowReduce rr;
  if (!p || p->layer < 0 || p->B < 1 || p->Lz < 0 || p->Lx < 1 || p->Lz + p->Lx > 1024 || !p->srcA || !p->w00 ||
      !p->b00 || !p->a8 || !p->c8 || !to_row_reduce(reduce, rr))
    return MMT_E_ARG;
  PromptArgs a{};
  if (p->layer == 0) {
    if (!p->srcB || !p->lnA_w || !p->lnA_b || !p->lnB_w || !p->lnB_b || !p->w01 || !p->b01 || rr.ws) return MMT_E_ARG;
    a.srcA_rows = p->Lz + p->Lx;
  } else {
    if (!p->slot2pos || !p->fold || !p->a8p || !p->c8p || p->srcA_rows < p->Lz || p->srcA_rows < 1) return MMT_E_ARG;
    const int r = check_index_list(p->slot2pos, (size_t)p->B * p->Lx, -1, p->srcA_rows);
    if (r) return r;
    a.srcA_rows = p->srcA_rows;
  }
  a.layer = p->layer;
  a.B = p->B;
  a.Lz = p->Lz;
  a.Lx = p->Lx;
  a.srcA = p->srcA;
  a.srcB = p->srcB;
  a.slot2pos = p->slot2pos;
  a.lnA_w = p->lnA_w;
  a.lnA_b = p->lnA_b;
  a.lnB_w = p->lnB_w;
  a.lnB_b = p->lnB_b;
  a.w00 = p->w00;
  a.b00 = p->b00;
  a.w01 = p->w01;
  a.b01 = p->b01;
  a.fold = p->fold;
  a.a8 = p->a8;
  a.c8 = p->c8;
  a.a8p = p->a8p;
  a.c8p = p->c8p;
  a.smooth_p = p->smooth_p;
  a.fstat_p = p->fstat_p;
  a.rr = rr;
  if (!prompt_reduce(a, (hipStream_t)stream)) return MMT_E_ARG;
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_prompt_expand_ln(const mmt_ln_prompt_args* p, void* stream) {
  if (!p || (p->mode != 1 && p->mode != 2) || p->rows < 1 || p->rows_per_seq < 1 || p->rows % p->rows_per_seq ||
      p->Lz < 0 || p->Lx < 1 || p->Lz + p->Lx > 1024 || !p->X || !p->a8 || !p->c8 || !p->w1 || !p->b1 || !p->w || !p->b ||
      !p->out)
    return MMT_E_ARG;
  if (p->mode == 1) {
    if (!p->tok_rgb || !p->pos || p->rows_per_seq != p->Lz + p->Lx) return MMT_E_ARG;
  } else {
    if (!p->gidx || p->rows_per_seq <= p->Lz || p->rows_per_seq > p->Lz + p->Lx) return MMT_E_ARG;
    const int r = check_index_list(p->gidx, (size_t)(p->rows / p->rows_per_seq) * (p->rows_per_seq - p->Lz), 0, p->Lx);
    if (r) return r;
  }
  LnPromptArgs a{};
  a.mode = p->mode;
  a.rows = p->rows;
  a.rows_per_seq = p->rows_per_seq;
  a.Lz = p->Lz;
  a.Lx = p->Lx;
  a.X = p->X;
  a.a8 = p->a8;
  a.c8 = p->c8;
  a.smooth = p->smooth;
  a.fstat = p->fstat;
  a.w1 = p->w1;
  a.b1 = p->b1;
  a.tok_rgb = p->tok_rgb;
  a.pos = p->pos;
  a.gidx = p->gidx;
  a.w = p->w;
  a.b = p->b;
  a.out = (bf16_t*)p->out;
  a.out_lo = (bf16_t*)p->out_lo;
  a.out_scale = p->out_scale;
  if (!prompt_expand_ln(a, (hipStream_t)stream)) return MMT_E_ARG;
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_prompt_fold(const float* conv0_0_w, const float* conv0_0_b, const float* ln_a_w, const float* ln_a_b,
                    const float* conv0_1_w, const float* conv0_1_b, const float* ln_b_w, const float* ln_b_b,
                    const float* conv1x1_prev_w, const float* conv1x1_prev_b, float* w00f, float* b00f, float* fold) {
  if (!conv0_0_w || !conv0_0_b || !ln_a_w || !ln_a_b || !conv0_1_w || !conv0_1_b || !ln_b_w || !ln_b_b ||
      !conv1x1_prev_w || !conv1x1_prev_b || !w00f || !b00f || !fold)
    return MMT_E_ARG;
  prompt_fold(conv0_0_w, conv0_0_b, ln_a_w, ln_a_b, conv0_1_w, conv0_1_b, ln_b_w, ln_b_b, conv1x1_prev_w,
              conv1x1_prev_b, w00f, b00f, fold);
  return MMT_OK;
}

}  // extern "C"
