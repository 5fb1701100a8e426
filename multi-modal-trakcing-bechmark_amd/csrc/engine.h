// The tracking engine's state, shared by engine.cpp (lifecycle, tracking ABI, graphs), engine_weights.cpp (state-dict
// layout and weight packing), engine_forward.cpp (the per-frame launch sequence) and ops_api.cpp (the stateless
// operator entry points).  Internal to csrc/: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/mmtrack.h"
#include "kernels.h"

namespace mmt {

constexpr int C = 768;
constexpr int HEADS = 12;
constexpr int DEPTH = 12;
constexpr int MLPD = 3072;
constexpr int kRing = MMT_PIPELINE_DEPTH;     // submitted-but-unfetched frames an engine holds
constexpr int64_t kSplitKWsElems = 4 << 20;   // 16 MB of fp32 split-K partials per launch part (and mmt_op_gemm*)

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

struct LayerW {
  bf16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
  bf16_t *qkv_wl, *proj_wl, *fc1_wl, *fc2_wl;   // low halves (fp32-faithful mode)
  float *qkv_b, *proj_b, *fc1_b, *fc2_b, *n1w, *n1b, *n2w, *n2b;
  // f16x3 range scales (powers of two, 1 in bf16 mode): weights, and the split activations this block
  // produces -- LN1 / LN2 outputs, qkv output (Q, K, V and the attention output O), fc1 (GELU) output
  float qkv_s = 1, proj_s = 1, fc1_s = 1, fc2_s = 1, ln1_s = 1, ln2_s = 1, qkv_os = 1, fc1_os = 1;
};

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

// The activation buffers: [max_batch] sequences each, carved from one zeroed arena (alloc_acts).  for_each_act below
// is their one description; the engine holds the base pointers and a launch part works on act_view(), a copy
// advanced to its first slot / launch row.
struct Acts {
  bf16_t *A_rgb, *A_aux, *Hn, *QKV, *O, *Hm, *feat, *h1, *h2, *h3;
  // low halves of every bf16 GEMM operand (fp32-faithful mode only, else null)
  bf16_t *A_rgb_l, *A_aux_l, *Hn_l, *QKV_l, *O_l, *Hm_l, *feat_l, *h1_l, *h2_l, *h3_l;
  // a8 / c8: the prompt blocks' two 8-channel branches, [2][B][L][8] each (layer i writes half i & 1 and the
  // next layer re-forms the fovea output s8 from the half it did not write)
  float *tok_rgb, *tok_aux, *X, *X2, *a8, *c8, *fstat, *h4, *ce_prob, *res;
  int *gidx0, *gidx1, *slot2pos, *gather, *removed;
  CropParam* params_dev;
  SeqState* state_dev;   // tracker state per slot (device-resident)
  TrackOut* out_dev;     // per-launch results
  // mask mode (cfg.ce_template_index = MMT_CE_TEMPLATE_MASK): per slot, the compact ascending list of the template
  // tokens whose attention rows score the search tokens ([max_batch][Lz]) and its length; every token (ALL) until
  // mmt_set_ce_template_mask.  Fixed device addresses: captured graphs read the lists' current contents.
  int *ce_rows, *ce_nrows;
  // parity diagnostics (debug_outputs): CE keys [B][n_ce][Lx] as computed, and teacher-forced keys
  float *ce_keys, *ce_forced, *dbg_maps, *dbg_feat;
  uint8_t* dbg_patch;
  size_t half8;   // floats between the two halves of a8 / c8
  float* a8_of(int layer) const { return a8 + (size_t)(layer & 1) * half8; }
  float* c8_of(int layer) const { return c8 + (size_t)(layer & 1) * half8; }
};
// what a launch part's view of a buffer is advanced by: its first slot (b0: what outlives a launch, by sequence
// slot) or its first launch row (r0: scratch of the launch, by position in the launch)
enum ActIndex { BY_SLOT, BY_ROW };
enum ActWhen { ALWAYS, IF_CE_MASK, IF_SPLIT, IF_DEBUG };   // the buffer exists: ..., e->ce_mask, e->split, debug_outputs

}  // namespace mmt

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
  std::map<std::string, mmt::HostTensor> host;
  bool finalized = false;

  // geometry
  int Lz = 0, Lx = 0, L = 0, fs = 0, tfs = 0;
  std::vector<int> ls_before;   // search tokens entering block i
  std::vector<int> keep_at;     // search tokens kept after block i (== ls_before[i] if no CE)

  // weights (one arena)
  void* warena = nullptr;
  size_t wcap = 0, wused = 0;
  mmt::LayerW lw[mmt::DEPTH];
  mmt::PromptW pw[mmt::DEPTH];
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
  mmt::Acts acts{};
  bf16_t* zero = nullptr;
  bool split = false;
  bool force_ce = false;   // debug_outputs: CE decides on acts.ce_forced
  bool ce_mask = false;
  float* splitk_ws = nullptr;   // [kMaxParts launch parts][kSplitKWsElems] fp32 split-K partials (few-tile GEMMs)
  mmt::CropParam* params_host = nullptr;   // pinned [kRing][max_batch]
  mmt::TrackOut* outs_host = nullptr;      // pinned [kRing][max_batch]
  // ring hand-off: the geometry kernel reads a launch's frame parameters straight from params_host and
  // the decode kernel writes its results straight into outs_host (device-visible pinned memory), so a
  // step carries no copy launches; the device counts executed launches (hring.ctr) exactly as `launches`
  // does on the host, and a ticket keeps the ring entry (launches % kRing) its launch used
  bool ring_handoff = true;
  mmt::RingArgs hring{};
  int64_t launches = 0;

  // pipelined frames (mmt_track_batch_submit / _fetch): ticket t uses ring entry t % kRing
  struct Ticket {
    int64_t id = -1;
    int first = 0, n = 0;
    bool open = false;
    hipEvent_t done = nullptr;
    const mmt::GraphEntry* replayed = nullptr;
    int entry = 0;   // params / results ring entry of its launch
  };
  Ticket ring[mmt::kRing];
  int64_t next_ticket = 0;
  int unfetched = 0;

  // host-frame staging: per (slot, ring entry) device copies, made on a copy stream so a pipelined
  // frame's PCIe transfer overlaps the compute of the frames before it
  std::vector<uint8_t*> frame_dev;     // [max_batch * kRing]
  std::vector<size_t> frame_cap;
  hipStream_t cstream = nullptr;
  hipEvent_t copy_ev[mmt::kRing] = {};
  hipStream_t frame_stream = nullptr;  // caller's stream that produces device frames (mmt_set_frame_stream;
  bool frame_wait = false;             // null = the legacy default stream)
  hipEvent_t frame_ev = nullptr;

  // tracker state (vipt.py:57, 88) in doubles
  std::vector<std::array<double, 4>> state;
  std::vector<char> active;
  int last_batch = 0;

  std::map<std::tuple<int, int, std::string>, mmt::GraphEntry> graphs;
  std::unique_ptr<mmt::TimingProbe> probe;

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
};

#define HIPCHECK(e, expr)                                                              \
  do {                                                                                 \
    hipError_t _st = (expr);                                                           \
    if (_st != hipSuccess)                                                             \
      return (e)->fail(MMT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_st)); \
  } while (0)

#define TRY(x)                   \
  do {                           \
    int _r = (x);                \
    if (_r != MMT_OK) return _r; \
  } while (0)

namespace mmt {

// The one table of the activation buffers: f(member, elements per sequence, what indexes it, when it exists, planes),
// in arena order within each ActWhen.  planes: a8 / c8 are [2][B][L][8], every other buffer one [B] plane.
template <class A, class F>
void for_each_act(A& a, const mmt_engine* e, F&& f) {
  const size_t L = e->L, Lx = e->Lx, Lz = e->Lz, hc = e->cfg.head_channels, S = e->cfg.search_size;
  const size_t nce = std::max(e->cfg.n_ce, 1);
  // a bf16 GEMM operand and, in the parity mode, its low half
  auto split = [&](auto& hi, auto& lo, size_t per, ActIndex ix) {
    f(hi, per, ix, ALWAYS, 1);
    f(lo, per, ix, IF_SPLIT, 1);
  };
  split(a.A_rgb, a.A_rgb_l, L * C, BY_SLOT);   // template rows are written at initialize, search rows per frame
  split(a.A_aux, a.A_aux_l, L * C, BY_SLOT);
  f(a.tok_rgb, L * C, BY_ROW, ALWAYS, 1);
  f(a.tok_aux, L * C, BY_ROW, ALWAYS, 1);
  f(a.X, L * C, BY_ROW, ALWAYS, 1);
  f(a.X2, L * C, BY_ROW, ALWAYS, 1);
  f(a.a8, L * 8, BY_ROW, ALWAYS, 2);
  f(a.fstat, 32, BY_ROW, ALWAYS, 1);
  f(a.c8, L * 8, BY_ROW, ALWAYS, 2);
  split(a.Hn, a.Hn_l, L * C, BY_ROW);
  split(a.QKV, a.QKV_l, L * 3 * C, BY_ROW);
  split(a.O, a.O_l, L * C, BY_ROW);
  split(a.Hm, a.Hm_l, L * MLPD, BY_ROW);
  split(a.feat, a.feat_l, Lx * C, BY_ROW);
  split(a.h1, a.h1_l, Lx * 3 * hc, BY_ROW);         // [M][3*hc]
  split(a.h2, a.h2_l, Lx * 3 * (hc / 2), BY_ROW);   // [3][M][hc/2], as h3 and h4
  split(a.h3, a.h3_l, Lx * 3 * (hc / 4), BY_ROW);
  f(a.h4, Lx * 3 * 32, BY_ROW, ALWAYS, 1);
  f(a.ce_prob, HEADS * Lx, BY_ROW, ALWAYS, 1);
  f(a.res, 8, BY_ROW, ALWAYS, 1);
  f(a.gidx0, Lx, BY_ROW, ALWAYS, 1);
  f(a.gidx1, Lx, BY_ROW, ALWAYS, 1);
  f(a.slot2pos, Lx, BY_ROW, ALWAYS, 1);
  f(a.gather, L, BY_ROW, ALWAYS, 1);
  f(a.removed, Lx, BY_ROW, ALWAYS, 1);
  f(a.params_dev, 1, BY_ROW, ALWAYS, 1);
  f(a.state_dev, 1, BY_SLOT, ALWAYS, 1);
  f(a.out_dev, 1, BY_ROW, ALWAYS, 1);
  f(a.ce_rows, Lz, BY_SLOT, IF_CE_MASK, 1);
  f(a.ce_nrows, 1, BY_SLOT, IF_CE_MASK, 1);
  f(a.ce_keys, nce * Lx, BY_ROW, IF_DEBUG, 1);   // [n_ce][Lx]: one row per CE stage
  f(a.ce_forced, nce * Lx, BY_SLOT, IF_DEBUG, 1);
  f(a.dbg_patch, S * S * e->cfg.in_chans, BY_ROW, IF_DEBUG, 1);
  f(a.dbg_maps, 5 * Lx, BY_ROW, IF_DEBUG, 1);
  f(a.dbg_feat, L * C, BY_ROW, IF_DEBUG, 1);
}

// the buffers as the launch part over slots [b0, ..) = launch rows [r0, ..) sees them (null stays null)
inline Acts act_view(const mmt_engine* e, int b0, int r0) {
  Acts v = e->acts;
  for_each_act(v, e, [&](auto*& p, size_t per, ActIndex ix, ActWhen, int) {
    if (p) p += (size_t)(ix == BY_SLOT ? b0 : r0) * per;
  });
  return v;
}

// bytes per sequence of the buffer whose base pointer is `base` (0: not a buffer of the table)
inline size_t act_bytes(const mmt_engine* e, const void* base) {
  size_t bytes = 0;
  for_each_act(e->acts, e, [&](auto* p, size_t per, ActIndex, ActWhen, int) {
    if (p && (const void*)p == base) bytes = per * sizeof(*p);
  });
  return bytes;
}

// engine_weights.cpp
void build_expected(mmt_engine* e);   // the reference's state_dict layout -> e->expected
int pack_weights(mmt_engine* e);      // e->host -> the weight arena (range scales, folds, f16x3 halves)
void prompt_fold(const float* W00, const float* b00, const float* gA, const float* bA, const float* W, const float* w0,
                 const float* g, const float* bb, const float* V, const float* v0, float* wf, float* bf, float* f);

// engine_forward.cpp
// One launch over n sequences from slot b0, on e->stream (and e->xstream for a split launch).  false: a GEMM of
// the launch has no kernel (e->err says which); the rest was enqueued all the same
bool enqueue_split(mmt_engine* e, int b0, int n);
void probe_collect(mmt_engine* e);
void probe_collect_graph(mmt_engine* e, const GraphEntry& g);

}  // namespace mmt
