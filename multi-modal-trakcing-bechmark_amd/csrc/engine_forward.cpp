// The per-frame launch sequence of the tracking engine: embed, twelve blocks, head, per launch part; the split of a
// launch into parts on separate streams; the kernel timing probe that brackets one class of these launches.
#include <algorithm>
#include <cstdlib>

#include "engine.h"

using namespace mmt;

namespace {

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

}  // namespace

void mmt::probe_collect_graph(mmt_engine* e, const GraphEntry& g) {
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

void mmt::probe_collect(mmt_engine* e) {
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

namespace {

// ---------------------------------------------------------------- the per-frame launch sequence
// What one launch part is made of: n sequences, slots [b0, b0 + n) = launch rows [r0, r0 + n), on one stream.
struct Launch {
  mmt_engine* e;
  hipStream_t s;
  int n, b0, r0;
  // split-K workspace per stream part; parity mode only (in bf16 a different summation order can flip a
  // bf16 rounding and, through CE, a box: that mode keeps batch-size-independent results instead)
  float* ws;
  Acts v;           // the activation buffers as this part sees them (act_view)
  bool fuse_geom;   // a launch not split into stream parts: the geometry kernel's work done by the crop itself
  bool ok = true;   // false: a launch of this part has no kernel (e->err says which); the rest was enqueued all the same
};

// What travels from one block to the next.
struct Flow {
  float *X, *X2;     // the residual stream, and the buffer CE compacts it into (they swap there)
  int *gin, *gout;   // slot of each compact search token: current, and CE's output (they swap too)
  int Ls;            // search tokens left
  int removed_off = 0, ce_stage = 0;
  // a split-K update of the residual stream X still in the workspace (proj / fc2 of few-tile launches): the next
  // row kernel that reads X applies it and writes X back, instead of a reduce launch
  RowReduce pend{};
  PromptArgs pa{};   // the prompt block's arguments, carried between the deep-prompt layers
};

// offset a possibly-null low-half pointer
template <class T>
inline T* off(T* p, size_t o) {
  return p ? p + o : nullptr;
}

GemmArgs dense(const Launch& lc, const GemmGroup& g, int M, int N, int K) {
  GemmArgs a{};
  a.g[0] = g;
  a.groups = 1;
  a.split = lc.e->split ? 1 : 0;
  a.zero = lc.e->zero;
  a.M = M;
  a.N = N;
  a.K = K;
  a.amode = A_DENSE;
  // GEMMs with few 64 x 64 tiles and a long K (small batches: fc2 / proj / head convs at one or two
  // sequences) split K over workgroups into this stream half's workspace, reduced in a fixed order with the
  // epilogue (gemm.hip).  The summation order then depends on the batch size: results agree across batch
  // sizes to fp32 rounding, not bit for bit (test_batch_equals_single).
  a.ws = lc.ws;
  a.ws_elems = lc.ws ? kSplitKWsElems : 0;
  a.conc = lc.e->conc_parts;
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
// runs this GEMM nothing is launched: -1, lc.ok = false and the reason in e->err
int run_gemm(Launch& lc, const char* cls, const GemmArgs& a, int epi) {
  const double flops = 2.0 * a.M * a.N * (double)a.K * a.groups;
  // algorithmic HBM bytes: A and W once, C once (bf16 or fp32), R once for the residual epilogues
  const bool out16 = epi == EPI_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RELU_BF16;
  const double outb = (double)a.M * a.N * (out16 ? 2.0 : 4.0) * (a.split && out16 ? 2.0 : 1.0);
  const double rb = (epi == EPI_RESID_F32) ? (double)a.M * a.N * 4.0 : 0.0;
  const double bytes = (((double)a.M * a.K + (double)a.N * a.K) * 2.0 * (a.split ? 2.0 : 1.0) + outb + rb) * a.groups;
  probe_begin(lc.e, lc.s, cls, flops, bytes);
  const char* why = nullptr;
  const int ks = gemm(a, epi, lc.s, &why);
  probe_end(lc.e, lc.s, cls);
  if (ks < 0) {
    lc.e->err = std::string("gemm ") + cls + ": " + why;
    lc.ok = false;
  }
  return ks;
}

// a token kernel's launcher declined (more than 1 024 search tokens / slots per sequence): nothing was launched
void token_fail(Launch& lc, const char* what) {
  lc.e->err = std::string(what) + ": more than 1024 tokens per sequence";
  lc.ok = false;
}

// a residual-stream GEMM (EPI_RESID_F32 into X) whose split-K combine is left to the consuming row kernel
RowReduce run_resid_gemm(Launch& lc, const char* cls, GemmArgs a) {
  a.defer_reduce = a.ws ? 1 : 0;
  const int ks = run_gemm(lc, cls, a, EPI_RESID_F32);
  RowReduce rr{};
  if (ks > 1) rr = RowReduce{a.ws, ks, (int64_t)a.M * a.N, a.g[0].inv, a.g[0].bias};
  return rr;
}

// the arguments of prompt block i, whose LN_A is prompt_norms[lnA]; the caller adds the sources
void set_prompt(const Launch& lc, PromptArgs& pa, int i, int lnA) {
  const mmt_engine* e = lc.e;
  pa.layer = i;
  pa.a8 = lc.v.a8_of(i);
  pa.c8 = lc.v.c8_of(i);
  pa.a8p = i ? lc.v.a8_of(i - 1) : nullptr;
  pa.c8p = i ? lc.v.c8_of(i - 1) : nullptr;
  pa.smooth_p = i ? e->pw[i - 1].smooth : 0.f;
  pa.fstat_p = i ? lc.v.fstat : nullptr;   // written by layer i-1's LN1 (prompt_expand_ln)
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
}

bool prompted(const mmt_config& c) { return c.model == MMT_MODEL_VIPT && c.prompt_type != MMT_PROMPT_NONE; }
bool deep_prompt(const mmt_config& c) { return c.model == MMT_MODEL_VIPT && c.prompt_type == MMT_PROMPT_DEEP; }

// crop + normalise + patchify, patch embedding, the layer-0 prompt
void embed(Launch& lc, Flow& f) {
  mmt_engine* e = lc.e;
  const auto& c = e->cfg;
  const Acts& v = lc.v;
  const int Lz = e->Lz, Lx = e->Lx, L = e->L, n = lc.n;
  // 1. (crop geometry: enqueue_split, once per launch) crop + normalise + patchify
  CropArgs ca{};
  ca.params = v.params_dev;
  ca.B = n;
  ca.out_sz = c.search_size;
  ca.C = c.in_chans;
  ca.A_rgb = v.A_rgb;
  ca.A_aux = v.A_aux;
  ca.A_rgb_lo = v.A_rgb_l;
  ca.A_aux_lo = v.A_aux_l;
  ca.rows_per_seq = L;
  ca.row0 = Lz;
  ca.dbg_patch = v.dbg_patch;
  if (lc.fuse_geom) {
    ca.geom.state = v.state_dev;
    ca.geom.factor = c.search_factor;
    ca.geom.ring = e->hring;
    ca.geom.use_ring = e->ring_handoff ? 1 : 0;
    ca.geom.gidx = v.gidx0;
    ca.geom.slot2pos = v.slot2pos;
    ca.geom.Lz = Lz;
    ca.geom.Lx = Lx;
  }
  crop_patchify(ca, lc.s);

  // 2. patch embedding (template rows were written at initialize)
  if (c.model == MMT_MODEL_VIPT) {
    GemmArgs g = dense(lc, {v.A_rgb, v.A_rgb_l, C, e->pe_w, e->pe_wl, C, e->pe_b, v.tok_rgb, nullptr, C, nullptr, 0},
                       n * L, C, C);
    g.g[1] = GemmGroup{v.A_aux, v.A_aux_l, C, e->pep_w, e->pep_wl, C, e->pep_b, v.tok_aux, nullptr, C, nullptr, 0};
    g.groups = 2;
    g = scaled(g, kPixScale * e->pe_s, 1.0f);
    g.g[1].inv = 1.0f / (kPixScale * e->pep_s);
    run_gemm(lc, "patch", g, EPI_F32);
  } else {
    GemmArgs g = dense(lc, {v.A_rgb, v.A_rgb_l, C, e->pe_w, e->pe_wl, C, e->pe_b, f.X, nullptr, C, e->pos, C},
                       n * L, C, C);
    g.pos_rows = L;
    run_gemm(lc, "patch", scaled(g, kPixScale * e->pe_s, 1.0f), EPI_POS_F32);
  }
  // (the token index arrays gidx0 / slot2pos were reset by the launch's geometry kernel, enqueue_split)

  f.pa.B = n;
  f.pa.Lz = Lz;
  f.pa.Lx = Lx;
  if (prompted(c)) {  // layer-0 prompt: vit_ce_prompt.py:205-219
    set_prompt(lc, f.pa, 0, 0);
    f.pa.srcA = v.tok_rgb;
    f.pa.srcA_rows = L;
    f.pa.srcB = v.tok_aux;
    f.pa.slot2pos = nullptr;
    // fovea, P and X = tok_rgb + P + pos are formed with block 0's LN1
    if (!prompt_reduce(f.pa, lc.s)) token_fail(lc, "prompt_reduce");
  }
}

// transformer block i: LN1 (with the prompt block of a prompted layer), qkv, attention, proj, LN2 (with candidate
// elimination where the block has it), fc1, fc2
void block(Launch& lc, Flow& f, int i) {
  mmt_engine* e = lc.e;
  const auto& c = e->cfg;
  const Acts& v = lc.v;
  const hipStream_t s = lc.s;
  const int Lz = e->Lz, Lx = e->Lx, n = lc.n;
  const LayerW& w = e->lw[i];
  const bool deep = deep_prompt(c);
  const int Na = Lz + f.Ls;
  int ln_mode = (prompted(c) && i == 0) ? 1 : 0;
  if (deep && i >= 1) {  // vit_ce_prompt.py:268-310
    set_prompt(lc, f.pa, i, i - 1);
    f.pa.srcA = f.X;
    f.pa.srcA_rows = Na;
    f.pa.srcB = nullptr;
    f.pa.slot2pos = v.slot2pos;
    f.pa.rr = f.pend;   // the previous block's fc2 update of X
    f.pend = RowReduce{};
    ln_mode = 2;    // prompt_reduce(pa) below, with LN1 or before it
  }
  if (ln_mode) {
    LnPromptArgs la{};
    la.mode = ln_mode;
    la.rows = n * Na;
    la.rows_per_seq = Na;
    la.Lz = Lz;
    la.Lx = Lx;
    la.X = f.X;
    la.a8 = v.a8_of(i);
    la.c8 = v.c8_of(i);
    la.smooth = e->pw[i].smooth;
    la.fstat = deep ? v.fstat : nullptr;   // read by layer i+1's prompt_reduce (PromptArgs::fstat_p)
    la.w1 = e->pw[i].w1;   // conv1x1 of the prompt block that ran for this layer
    la.b1 = e->pw[i].b1;
    la.tok_rgb = v.tok_rgb;
    la.pos = e->pos;
    la.gidx = f.gin;
    la.w = w.n1w;
    la.b = w.n1b;
    la.out = v.Hn;
    la.out_lo = v.Hn_l;
    la.out_scale = w.ln1_s;
    if (ln_mode == 2 && !prompt_reduce(f.pa, s)) token_fail(lc, "prompt_reduce");
    if (!prompt_expand_ln(la, s)) token_fail(lc, "prompt_expand_ln");
  } else {
    layernorm(f.X, w.n1w, w.n1b, v.Hn, v.Hn_l, w.ln1_s, nullptr, n * Na, Na, nullptr, Na, nullptr, s, f.pend);
    f.pend = RowReduce{};
  }
  run_gemm(lc, "qkv",
           scaled(dense(lc, {v.Hn, v.Hn_l, C, w.qkv_w, w.qkv_wl, C, w.qkv_b, v.QKV, v.QKV_l, 3 * C, nullptr, 0}, n * Na,
                        3 * C, C),
                  w.ln1_s * w.qkv_s, w.qkv_os),
           EPI_BF16);
  const bool ce = e->keep_at[i] != e->ls_before[i];
  AttnArgs aa{};
  aa.qkv = v.QKV;
  aa.qkv_lo = v.QKV_l;
  aa.out = v.O;
  aa.out_lo = v.O_l;
  aa.qk_inv = 0.125f / (w.qkv_os * w.qkv_os);   // attn.py:15 scale 64^-0.5
  aa.pv_inv = 1.0f / (16384.0f * w.qkv_os);
  aa.out_scale = w.qkv_os;                      // |O| <= max |V|
  aa.B = n;
  aa.N = Na;
  aa.heads = HEADS;
  aa.ce_query = ce && !e->ce_mask ? c.ce_template_index : -1;
  aa.ce_lens_t = Lz;
  aa.ce_prob = v.ce_prob;
  // algorithmic bytes: Q, K, V in and O out, 2 B per element, twice in the parity mode (hi + lo planes: 12 288 B per
  // token row), as the GEMM classes count their operands
  probe_begin(e, s, "attn", 4.0 * n * HEADS * (double)Na * Na * 64, (double)n * Na * 4 * C * 2 * (e->split ? 2 : 1));
  attention(aa, s);
  probe_end(e, s, "attn");
  if (ce && e->ce_mask) {   // the mean over the slots' template masks instead of attention's single exported row
    CeRowsArgs cr{};
    cr.qkv = v.QKV;
    cr.qkv_lo = v.QKV_l;
    cr.B = n;
    cr.N = Na;
    cr.heads = HEADS;
    cr.lens_t = Lz;
    cr.rows = v.ce_rows;
    cr.pitch = Lz;
    cr.nrows = v.ce_nrows;
    cr.prob = v.ce_prob;
    cr.qk_inv = aa.qk_inv;
    // at most Lz rows against Na keys, twice (the search-key tiles are multiplied again): K of every head once
    probe_begin(e, s, "ce_rows", 2.0 * n * HEADS * (double)Lz * (2.0 * Na - Lz) * 64,
                (double)n * Na * C * 2 * (e->split ? 2 : 1));
    ce_rows(cr, s);
    probe_end(e, s, "ce_rows");
  }
  f.pend = run_resid_gemm(
      lc, "proj",
      scaled(dense(lc, {v.O, v.O_l, C, w.proj_w, w.proj_wl, C, w.proj_b, f.X, nullptr, C, f.X, C}, n * Na, C, C),
             w.qkv_os * w.proj_s, 1.0f));
  if (ce) {  // attn_blocks.py:99-101
    const int keep = e->keep_at[i];
    CEArgs ce_a{};
    ce_a.B = n;
    ce_a.Lz = Lz;
    ce_a.Ls = f.Ls;
    ce_a.keep = keep;
    ce_a.heads = HEADS;
    ce_a.Lx = Lx;
    ce_a.prob = v.ce_prob;
    ce_a.gidx_in = f.gin;
    ce_a.gidx_out = f.gout;
    ce_a.gather = v.gather;
    ce_a.slot2pos = v.slot2pos;
    ce_a.removed = v.removed;
    ce_a.removed_off = f.removed_off;
    ce_a.keys_pitch = std::max(c.n_ce, 1) * Lx;   // ce_keys / ce_forced: [n_ce][Lx] per sequence, one row per CE stage
    ce_a.keys_out = off(v.ce_keys, (size_t)f.ce_stage * Lx);
    ce_a.forced = e->force_ce ? off(v.ce_forced, (size_t)f.ce_stage * Lx) : nullptr;
    ++f.ce_stage;
    if (!ce_layernorm(ce_a, f.X, w.n2w, w.n2b, v.Hn, v.Hn_l, w.ln2_s, Na, f.X2, s, f.pend)) {
      if (!ce_select(ce_a, s)) token_fail(lc, "ce_select");
      layernorm(f.X, w.n2w, w.n2b, v.Hn, v.Hn_l, w.ln2_s, nullptr, n * (Lz + keep), Lz + keep, v.gather, Na, f.X2, s,
                f.pend);
    }
    f.removed_off += f.Ls - keep;
    std::swap(f.gin, f.gout);
    f.Ls = keep;
    std::swap(f.X, f.X2);
  } else {
    layernorm(f.X, w.n2w, w.n2b, v.Hn, v.Hn_l, w.ln2_s, nullptr, n * Na, Na, nullptr, Na, nullptr, s, f.pend);
  }
  f.pend = RowReduce{};
  const int Nm = Lz + f.Ls;
  run_gemm(lc, "fc1",
           scaled(dense(lc, {v.Hn, v.Hn_l, C, w.fc1_w, w.fc1_wl, C, w.fc1_b, v.Hm, v.Hm_l, MLPD, nullptr, 0}, n * Nm,
                        MLPD, C),
                  w.ln2_s * w.fc1_s, w.fc1_os),
           EPI_GELU_BF16);
  f.pend = run_resid_gemm(
      lc, "fc2",
      scaled(dense(lc, {v.Hm, v.Hm_l, MLPD, w.fc2_w, w.fc2_wl, MLPD, w.fc2_b, f.X, nullptr, C, f.X, C}, n * Nm, C, MLPD),
             w.fc1_os * w.fc2_s, 1.0f));
}

// final norm + token recovery, the CENTER head, decode
void head(Launch& lc, Flow& f) {
  mmt_engine* e = lc.e;
  const auto& c = e->cfg;
  const Acts& v = lc.v;
  const int n = lc.n, Lx = e->Lx;
  final_norm_recover(f.X, e->Lz + f.Ls, v.slot2pos, e->norm_w, e->norm_b, n, e->Lz, Lx, v.feat, v.feat_l, e->feat_s,
                     v.dbg_feat, lc.s, f.pend);

  // conv1 of the three branches fused (N = 3*hc), then per-branch grouped convs
  const int hc = c.head_channels, fs = e->fs, M = n * Lx;
  {
    GemmArgs g = dense(lc, {v.feat, v.feat_l, C, e->hw1, e->hw1l, 9 * C, e->hb1, v.h1, v.h1_l, 3 * hc, nullptr, 0}, M,
                       3 * hc, 9 * C);
    g.amode = A_CONV3;
    g.conv_hw = fs;
    g.conv_cin = C;
    run_gemm(lc, "conv1", scaled(g, e->feat_s * e->hw1_s, e->h_s[0]), EPI_RELU_BF16);
  }
  // h1 is [M][3*hc] (conv1's output columns are the three branches side by side); h2..h4 are [3][M][c] (one plane
  // per branch), h4 in fp32 and without a low half
  char* const h[4] = {(char*)v.h1, (char*)v.h2, (char*)v.h3, (char*)v.h4};
  char* const h_l[4] = {(char*)v.h1_l, (char*)v.h2_l, (char*)v.h3_l, nullptr};
  const int ch[4] = {hc, hc / 2, hc / 4, hc / 8};
  const char* const cls[3] = {"conv2", "conv3", "conv4"};
  for (int j = 0; j < 3; ++j) {   // conv2, conv3, conv4: h[j] -> h[j + 1]
    const int ci = ch[j], co = ch[j + 1];
    const size_t wk = (size_t)co * 9 * ci, osz = j == 2 ? 4 : 2;   // a branch's weights; bytes of an output element
    bf16_t *const hw = e->hw[j], *const hwl = e->hwl[j];
    GemmArgs g = dense(lc, GemmGroup{}, M, co, 9 * ci);
    for (int k = 0; k < 3; ++k) {
      // conv2's input is branch k's columns of h1 (lda = 3*hc); after it, branch k's plane
      const size_t ia = 2 * (j == 0 ? (size_t)k * hc : (size_t)k * M * ci), oc = osz * k * M * co;
      g.g[k] = GemmGroup{(bf16_t*)(h[j] + ia), (bf16_t*)off(h_l[j], ia), j == 0 ? 3 * hc : ci,
                         hw + k * wk, off(hwl, k * wk), 9 * ci, e->hb[j] + k * co,
                         h[j + 1] + oc, off(h_l[j + 1], oc), co, nullptr, 0};
    }
    g.groups = 3;
    g.amode = A_CONV3;
    g.conv_hw = fs;
    g.conv_cin = ci;
    run_gemm(lc, cls[j], scaled(g, e->h_s[j] * e->hw_s[j], j < 2 ? e->h_s[j + 1] : 1.0f),
             j == 2 ? EPI_RELU_F32 : EPI_RELU_BF16);
  }
  DecodeArgs da{};
  da.B = n;
  da.fs = fs;
  da.h4 = v.h4;
  da.w5 = e->w5;
  da.b5 = e->b5;
  da.hann = e->hann;
  da.res = v.res;
  da.maps = v.dbg_maps;
  da.state = v.state_dev;
  da.params = v.params_dev;
  da.out = v.out_dev;
  da.search_size = c.search_size;
  if (e->ring_handoff) {
    da.ring_outs = e->hring.outs;
    da.ring_cur = e->hring.cur;
    da.ring_pitch = e->hring.pitch;
    da.row0 = lc.r0;
    if (lc.fuse_geom) {
      da.ring_ctr = e->hring.ctr;
      da.ring_kring = e->hring.kring;
    }
  }
  decode(da, lc.s);
}

// one launch part; false: a GEMM of it has no kernel (e->err says which); the rest was enqueued all the same
bool enqueue_forward(mmt_engine* e, int b0, int r0, int n, hipStream_t s, int part, bool fuse_geom) {
  Launch lc{e, s, n, b0, r0, e->split ? e->splitk_ws + (size_t)part * kSplitKWsElems : nullptr, act_view(e, b0, r0),
            fuse_geom};
  Flow f{lc.v.X, lc.v.X2, lc.v.gidx0, lc.v.gidx1, e->Lx};
  embed(lc, f);
  for (int i = 0; i < DEPTH; ++i) block(lc, f, i);
  head(lc, f);
  return lc.ok;
}

}  // namespace

// One launch over n sequences.  Batches of >= overlap_min sequences run as two independent halves on
// two streams (fork/join events, also valid inside stream capture): the halves' kernels overlap, so one
// half's latency-bound kernels (LayerNorm, prompt, CE select, head tails) fill the CUs the other
// half's GEMM tails leave idle.  Each half owns disjoint activation rows, results are unchanged.
bool mmt::enqueue_split(mmt_engine* e, int b0, int n) {
  // crop geometry of all n sequences from their device-resident state (and, ring hand-off, their frame
  // parameters from the host ring), once per launch before any part starts
  const Acts v = act_view(e, b0, 0);
  auto geometry_kernel = [&] {
    crop_geometry(v.params_dev, v.state_dev, n, e->cfg.search_factor, e->cfg.search_size,
                  e->ring_handoff ? &e->hring : nullptr, v.gidx0, v.slot2pos, e->Lz, e->Lx, e->stream);
  };
  if (e->overlap_min <= 0 || n < e->overlap_min || e->probe) {
    // one stream: the crop forms the geometry itself (MMT_GEOM_KERNEL, tuning: the separate geometry kernel)
    static const bool geom_kernel = getenv("MMT_GEOM_KERNEL") != nullptr;
    if (geom_kernel) geometry_kernel();
    return enqueue_forward(e, b0, 0, n, e->stream, 0, !geom_kernel);
  }
  geometry_kernel();
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
