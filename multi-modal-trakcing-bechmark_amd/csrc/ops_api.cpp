// C ABI of the stateless operator entry points (include/mmtrack.h: mmt_xcorr*, mmt_siamfc_*, mmt_op_*, the tuning
// switches, mmt_prompt_fold): one kernel launcher each, no engine.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "engine.h"

using namespace mmt;

namespace {

// a split-K workspace of the engine's size for the operator entry points (zeroed once); null: the GEMM runs unsplit
float* op_workspace() {
  static float* ws = nullptr;
  if (!ws && hipMalloc(&ws, kSplitKWsElems * 4) == hipSuccess && hipMemset(ws, 0, kSplitKWsElems * 4) != hipSuccess) {
    hipFree(ws);
    ws = nullptr;
  }
  return ws;
}

// their zero page (GemmArgs::zero)
const bf16_t* op_zero_page() {
  static bf16_t* zero = nullptr;
  if (!zero && hipMalloc(&zero, 256) == hipSuccess) hipMemset(zero, 0, 256);
  return zero;
}

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

int siamfc_crop_impl(const uint8_t* frame, int Hh, int Ww, int Cc, int64_t row_stride, int n, const int* y0,
                     const int* x0, const int* size, const int pad[3], int out_sz, float* out, int nhwc, void* stream) {
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

// ---- frame-side kernels: the C structs of include/mmtrack.h are the kernels' own (kernels.h), field for field
#define SAME_FIELD(CT, KT, f) \
  static_assert(offsetof(CT, f) == offsetof(KT, f) && sizeof(CT::f) == sizeof(KT::f), #CT "." #f)
static_assert(sizeof(mmt_crop_param) == sizeof(CropParam), "mmt_crop_param");
SAME_FIELD(mmt_crop_param, CropParam, frame);
SAME_FIELD(mmt_crop_param, CropParam, stride);
SAME_FIELD(mmt_crop_param, CropParam, H);
SAME_FIELD(mmt_crop_param, CropParam, W);
SAME_FIELD(mmt_crop_param, CropParam, C);
SAME_FIELD(mmt_crop_param, CropParam, x1);
SAME_FIELD(mmt_crop_param, CropParam, y1);
SAME_FIELD(mmt_crop_param, CropParam, crop_sz);
static_assert(sizeof(mmt_seq_state) == sizeof(SeqState), "mmt_seq_state");
SAME_FIELD(mmt_seq_state, SeqState, box);
SAME_FIELD(mmt_seq_state, SeqState, rf);
SAME_FIELD(mmt_seq_state, SeqState, err);
static_assert(sizeof(mmt_track_out) == sizeof(TrackOut), "mmt_track_out");
SAME_FIELD(mmt_track_out, TrackOut, box);
SAME_FIELD(mmt_track_out, TrackOut, score);
SAME_FIELD(mmt_track_out, TrackOut, err);
static_assert(sizeof(mmt_gemm_group) == sizeof(GemmGroup), "mmt_gemm_group");
SAME_FIELD(mmt_gemm_group, GemmGroup, A_lo);
SAME_FIELD(mmt_gemm_group, GemmGroup, W_lo);
SAME_FIELD(mmt_gemm_group, GemmGroup, bias);
SAME_FIELD(mmt_gemm_group, GemmGroup, C_lo);
SAME_FIELD(mmt_gemm_group, GemmGroup, R);
SAME_FIELD(mmt_gemm_group, GemmGroup, ldr);
SAME_FIELD(mmt_gemm_group, GemmGroup, inv);
SAME_FIELD(mmt_gemm_group, GemmGroup, out_scale);
static_assert(sizeof(mmt_siamfc_state) == sizeof(SiamState) && sizeof(mmt_siamfc_state) == 64, "mmt_siamfc_state");
SAME_FIELD(mmt_siamfc_state, SiamState, center);
SAME_FIELD(mmt_siamfc_state, SiamState, target_sz);
SAME_FIELD(mmt_siamfc_state, SiamState, z_sz);
SAME_FIELD(mmt_siamfc_state, SiamState, x_sz);
SAME_FIELD(mmt_siamfc_state, SiamState, pad);
SAME_FIELD(mmt_siamfc_state, SiamState, frame_num);
static_assert(sizeof(mmt_siamfc_params) == sizeof(SiamParams), "mmt_siamfc_params");
SAME_FIELD(mmt_siamfc_params, SiamParams, scale_num);
SAME_FIELD(mmt_siamfc_params, SiamParams, instance_sz);
SAME_FIELD(mmt_siamfc_params, SiamParams, response_sz);
SAME_FIELD(mmt_siamfc_params, SiamParams, response_up);
SAME_FIELD(mmt_siamfc_params, SiamParams, total_stride);
SAME_FIELD(mmt_siamfc_params, SiamParams, scale_penalty);
SAME_FIELD(mmt_siamfc_params, SiamParams, scale_factors);
SAME_FIELD(mmt_siamfc_params, SiamParams, scale_lr);
SAME_FIELD(mmt_siamfc_params, SiamParams, window_influence);
SAME_FIELD(mmt_siamfc_params, SiamParams, hann_sum);
static_assert(sizeof(mmt_siamfc_result) == sizeof(SiamResult), "mmt_siamfc_result");
SAME_FIELD(mmt_siamfc_result, SiamResult, box);
SAME_FIELD(mmt_siamfc_result, SiamResult, value);
SAME_FIELD(mmt_siamfc_result, SiamResult, scale_id);
SAME_FIELD(mmt_siamfc_result, SiamResult, row);
SAME_FIELD(mmt_siamfc_result, SiamResult, col);
SAME_FIELD(mmt_siamfc_result, SiamResult, err);
static_assert(sizeof(mmt_dimp_frame) == sizeof(SiamFrame), "mmt_dimp_frame");
SAME_FIELD(mmt_dimp_frame, SiamFrame, data);
SAME_FIELD(mmt_dimp_frame, SiamFrame, stride);
SAME_FIELD(mmt_dimp_frame, SiamFrame, H);
SAME_FIELD(mmt_dimp_frame, SiamFrame, W);
SAME_FIELD(mmt_dimp_frame, SiamFrame, C);
#undef SAME_FIELD

// the fields of mmt_siamfc_params a pooled SiamFC launch sizes its grid and its indexing from
bool siamfc_params_ok(const mmt_siamfc_params* p, int n) {
  return p && n > 0 && p->scale_num >= 1 && p->scale_num <= 8 && (int64_t)n * p->scale_num <= 65535 &&
         p->instance_sz >= 1 && p->instance_sz <= 4096 && p->response_sz >= 2 && p->response_sz <= 256 &&
         p->response_up >= 1 && (int64_t)p->response_up * p->response_sz <= 8192 && p->total_stride >= 1 &&
         p->hann_sum > 0;
}

const CropParam* kp(const mmt_crop_param* p) { return reinterpret_cast<const CropParam*>(p); }
CropParam* kp(mmt_crop_param* p) { return reinterpret_cast<CropParam*>(p); }
SeqState* ks(mmt_seq_state* p) { return reinterpret_cast<SeqState*>(p); }
TrackOut* ko(mmt_track_out* p) { return reinterpret_cast<TrackOut*>(p); }

// one int of device (or pinned) memory, read back; false: the copy failed
bool read_int(const int* dev, int& v) { return hipMemcpy(&v, dev, sizeof(int), hipMemcpyDefault) == hipSuccess; }

// the ring of an operator-level call: its fields, and the counter read back (`which`: ctr or cur) within [0, kring);
// entry: that counter
int check_ring(const mmt_ring_args& r, const int* which, int rows, int& entry) {
  if (!r.params || !r.ctr || !r.cur || !which || r.kring < 1 || r.pitch < rows) return MMT_E_ARG;
  if (!read_int(which, entry)) return MMT_E_HIP;
  return entry < 0 || entry >= r.kring ? MMT_E_ARG : MMT_OK;
}

RingArgs to_ring(const mmt_ring_args& r) {
  return RingArgs{kp(r.params), ko(r.outs), r.ctr, r.cur, r.kring, r.pitch};
}

// the frame fields of n descriptors, read back: a frame the kernel can index (C: the launch's channels, 0: 3 or 6)
int check_frames(const mmt_crop_param* dev, int n, int C, bool geometry_too) {
  std::vector<mmt_crop_param> h(n);
  if (hipMemcpy(h.data(), dev, (size_t)n * sizeof(mmt_crop_param), hipMemcpyDefault) != hipSuccess) return MMT_E_HIP;
  for (const mmt_crop_param& p : h) {
    if (!p.frame || p.H < 2 || p.W < 2 || (C ? p.C != C : (p.C != 3 && p.C != 6)) || p.stride < (int64_t)p.W * p.C)
      return MMT_E_ARG;
    if (geometry_too && (p.crop_sz < 1 || p.crop_sz > 1000000 || std::abs((int64_t)p.x1) > (1 << 28) ||
                         std::abs((int64_t)p.y1) > (1 << 28)))
      return MMT_E_ARG;
  }
  return MMT_OK;
}

}  // namespace

extern "C" {

int mmt_crop_geometry_host(const double box[4], double factor, int out_sz, int* x1, int* y1, int* crop_sz,
                           double* rf) {
#pragma clang fp contract(off)
  if (!box || !x1 || !y1 || !crop_sz || !rf) return MMT_E_ARG;
  const double x = box[0], y = box[1], w = box[2], h = box[3];
  const double cs = std::ceil(std::sqrt(w * h) * factor);
  const int err = !(cs >= 1.0) ? MMT_E_BOX : cs > 1e6 ? MMT_E_ARG : MMT_OK;
  if (err) {   // the harmless crop of geometry_of (imaging.hip)
    *x1 = *y1 = 0;
    *crop_sz = 1;
    *rf = 1.0;
    return err;
  }
  *crop_sz = (int)cs;
  *x1 = (int)std::nearbyint(x + 0.5 * w - cs * 0.5);   // half to even, as python's round
  *y1 = (int)std::nearbyint(y + 0.5 * h - cs * 0.5);
  *rf = (double)out_sz / cs;
  return MMT_OK;
}

int mmt_op_crop_geometry(mmt_crop_param* params, mmt_seq_state* state, int n, double factor, int out_sz,
                         const mmt_ring_args* ring, int* gidx, int* slot2pos, int Lz, int Lx, void* stream) {
  if (!params || !state || n < 1 || !(factor > 0) || out_sz < 1 || !gidx != !slot2pos ||
      (gidx && (Lz < 0 || Lx < 1 || (int64_t)n * Lx > 0x7fffffff)))
    return MMT_E_ARG;
  RingArgs r{};
  if (ring) {
    int e;
    const int rc = check_ring(*ring, ring->ctr, n, e);
    if (rc) return rc;
    r = to_ring(*ring);
  }
  crop_geometry(kp(params), ks(state), n, factor, out_sz, ring ? &r : nullptr, gidx, slot2pos, Lz, Lx,
                (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_crop_patchify(const mmt_crop_args* c, const mmt_geom_args* g, void* stream) {
  if (!c || !c->params || !c->A_rgb || c->B < 1 || c->out_sz < 16 || c->out_sz % 16 || c->out_sz > 4096 ||
      (c->C != 3 && c->C != 6) || (c->C == 6 && (!c->A_aux || !c->A_rgb_lo != !c->A_aux_lo)) || c->row0 < 0 ||
      c->rows_per_seq < 1 || c->row0 + (int64_t)(c->out_sz / 16) * (c->out_sz / 16) > c->rows_per_seq)
    return MMT_E_ARG;
  CropArgs a{};
  const mmt_crop_param* frames = c->params;
  if (g) {
    if (!g->state || !(g->factor > 0) || !g->gidx != !g->slot2pos ||
        (g->gidx && (g->Lz < 0 || g->Lx < 1 || (int64_t)c->B * g->Lx > 0x7fffffff)))
      return MMT_E_ARG;
    a.geom.state = ks(g->state);
    a.geom.factor = g->factor;
    a.geom.use_ring = g->use_ring ? 1 : 0;
    if (g->use_ring) {
      int e;
      const int rc = check_ring(g->ring, g->ring.ctr, c->B, e);
      if (rc) return rc;
      a.geom.ring = to_ring(g->ring);
      frames = g->ring.params + (int64_t)e * g->ring.pitch;
    }
    a.geom.gidx = g->gidx;
    a.geom.slot2pos = g->slot2pos;
    a.geom.Lz = g->Lz;
    a.geom.Lx = g->Lx;
  }
  const int rc = check_frames(frames, c->B, c->C, !g);
  if (rc) return rc;
  a.params = kp(c->params);
  a.B = c->B;
  a.out_sz = c->out_sz;
  a.C = c->C;
  a.A_rgb = (bf16_t*)c->A_rgb;
  a.A_aux = (bf16_t*)c->A_aux;
  a.A_rgb_lo = (bf16_t*)c->A_rgb_lo;
  a.A_aux_lo = (bf16_t*)c->A_aux_lo;
  a.rows_per_seq = c->rows_per_seq;
  a.row0 = c->row0;
  a.dbg_patch = c->dbg_patch;
  crop_patchify(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_decode(const mmt_decode_args* d, void* stream) {
  if (!d || d->B < 1 || d->fs < 1 || d->fs > 1024 || !d->h4 || !d->w5 || !d->b5 || !d->hann || !d->res)
    return MMT_E_ARG;
  if (d->state && (!d->params || !d->out || d->search_size < 1)) return MMT_E_ARG;
  if (d->ring_outs || d->ring_ctr) {   // the entry decode writes / advances from, read back
    if (!d->ring_cur || d->ring_kring < 1 || (d->ring_outs && (!d->state || d->row0 < 0 || d->row0 + d->B > d->ring_pitch)))
      return MMT_E_ARG;
    int e;
    if (!read_int(d->ring_cur, e)) return MMT_E_HIP;
    if (e < 0 || e >= d->ring_kring) return MMT_E_ARG;
  }
  DecodeArgs a{};
  a.B = d->B;
  a.fs = d->fs;
  a.h4 = d->h4;
  a.w5 = d->w5;
  a.b5 = d->b5;
  a.hann = d->hann;
  a.res = d->res;
  a.maps = d->maps;
  a.state = ks(d->state);
  a.params = kp(d->params);
  a.out = ko(d->out);
  a.search_size = d->search_size;
  a.ring_outs = ko(d->ring_outs);
  a.ring_cur = d->ring_cur;
  a.ring_pitch = d->ring_pitch;
  a.row0 = d->row0;
  a.ring_ctr = d->ring_ctr;
  a.ring_kring = d->ring_kring;
  decode(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_struct_layout(int which, size_t* out, int cap) {
  std::vector<size_t> v;
#define F(T, f) v.push_back(offsetof(T, f))
  switch (which) {
    case 0:
      v.push_back(sizeof(mmt_crop_param));
      F(mmt_crop_param, frame); F(mmt_crop_param, stride); F(mmt_crop_param, H); F(mmt_crop_param, W);
      F(mmt_crop_param, C); F(mmt_crop_param, x1); F(mmt_crop_param, y1); F(mmt_crop_param, crop_sz);
      F(mmt_crop_param, pad_);
      break;
    case 1:
      v.push_back(sizeof(mmt_seq_state));
      F(mmt_seq_state, box); F(mmt_seq_state, rf); F(mmt_seq_state, err); F(mmt_seq_state, pad_);
      break;
    case 2:
      v.push_back(sizeof(mmt_track_out));
      F(mmt_track_out, box); F(mmt_track_out, score); F(mmt_track_out, err); F(mmt_track_out, pad_);
      break;
    case 3:
      v.push_back(sizeof(mmt_ring_args));
      F(mmt_ring_args, params); F(mmt_ring_args, outs); F(mmt_ring_args, ctr); F(mmt_ring_args, cur);
      F(mmt_ring_args, kring); F(mmt_ring_args, pitch);
      break;
    case 4:
      v.push_back(sizeof(mmt_crop_args));
      F(mmt_crop_args, params); F(mmt_crop_args, B); F(mmt_crop_args, out_sz); F(mmt_crop_args, C);
      F(mmt_crop_args, A_rgb); F(mmt_crop_args, A_aux); F(mmt_crop_args, A_rgb_lo); F(mmt_crop_args, A_aux_lo);
      F(mmt_crop_args, rows_per_seq); F(mmt_crop_args, row0); F(mmt_crop_args, dbg_patch);
      break;
    case 5:
      v.push_back(sizeof(mmt_geom_args));
      F(mmt_geom_args, state); F(mmt_geom_args, factor); F(mmt_geom_args, ring); F(mmt_geom_args, use_ring);
      F(mmt_geom_args, gidx); F(mmt_geom_args, slot2pos); F(mmt_geom_args, Lz); F(mmt_geom_args, Lx);
      break;
    case 6:
      v.push_back(sizeof(mmt_decode_args));
      F(mmt_decode_args, B); F(mmt_decode_args, fs); F(mmt_decode_args, h4); F(mmt_decode_args, w5);
      F(mmt_decode_args, b5); F(mmt_decode_args, hann); F(mmt_decode_args, res); F(mmt_decode_args, maps);
      F(mmt_decode_args, state); F(mmt_decode_args, params); F(mmt_decode_args, out);
      F(mmt_decode_args, search_size); F(mmt_decode_args, ring_outs); F(mmt_decode_args, ring_cur);
      F(mmt_decode_args, ring_pitch); F(mmt_decode_args, row0); F(mmt_decode_args, ring_ctr);
      F(mmt_decode_args, ring_kring);
      break;
    case 7:
      v.push_back(sizeof(mmt_gemm_group));
      F(mmt_gemm_group, A); F(mmt_gemm_group, A_lo); F(mmt_gemm_group, lda); F(mmt_gemm_group, W);
      F(mmt_gemm_group, W_lo); F(mmt_gemm_group, ldw); F(mmt_gemm_group, bias); F(mmt_gemm_group, C);
      F(mmt_gemm_group, C_lo); F(mmt_gemm_group, ldc); F(mmt_gemm_group, R); F(mmt_gemm_group, ldr);
      F(mmt_gemm_group, inv); F(mmt_gemm_group, out_scale);
      break;
    case 8:
      v.push_back(sizeof(mmt_gemm_ex_args));
      F(mmt_gemm_ex_args, g); F(mmt_gemm_ex_args, groups); F(mmt_gemm_ex_args, M); F(mmt_gemm_ex_args, N);
      F(mmt_gemm_ex_args, K); F(mmt_gemm_ex_args, epi); F(mmt_gemm_ex_args, split); F(mmt_gemm_ex_args, conv_hw);
      F(mmt_gemm_ex_args, conv_cin); F(mmt_gemm_ex_args, pos_rows); F(mmt_gemm_ex_args, conc);
      F(mmt_gemm_ex_args, defer_reduce); F(mmt_gemm_ex_args, ws); F(mmt_gemm_ex_args, ws_elems);
      break;
    case 9:
      v.push_back(sizeof(mmt_gemm_ran));
      F(mmt_gemm_ran, tile); F(mmt_gemm_ran, ksplit); F(mmt_gemm_ran, deferred);
      break;
    case 10:
      v.push_back(sizeof(mmt_siamfc_state));
      F(mmt_siamfc_state, center); F(mmt_siamfc_state, target_sz); F(mmt_siamfc_state, z_sz); F(mmt_siamfc_state, x_sz);
      F(mmt_siamfc_state, pad); F(mmt_siamfc_state, frame_num);
      break;
    case 11:
      v.push_back(sizeof(mmt_siamfc_params));
      F(mmt_siamfc_params, scale_num); F(mmt_siamfc_params, instance_sz); F(mmt_siamfc_params, response_sz);
      F(mmt_siamfc_params, response_up); F(mmt_siamfc_params, total_stride); F(mmt_siamfc_params, scale_penalty);
      F(mmt_siamfc_params, scale_factors); F(mmt_siamfc_params, scale_lr); F(mmt_siamfc_params, window_influence);
      F(mmt_siamfc_params, hann_sum);
      break;
    case 12:
      v.push_back(sizeof(mmt_siamfc_result));
      F(mmt_siamfc_result, box); F(mmt_siamfc_result, value); F(mmt_siamfc_result, scale_id); F(mmt_siamfc_result, row);
      F(mmt_siamfc_result, col); F(mmt_siamfc_result, err); F(mmt_siamfc_result, pad_);
      break;
    case 13:
      v.push_back(sizeof(mmt_iounet_head));
      F(mmt_iounet_head, w3); F(mmt_iounet_head, b3); F(mmt_iounet_head, w4); F(mmt_iounet_head, b4);
      F(mmt_iounet_head, wp); F(mmt_iounet_head, bp); F(mmt_iounet_head, c3); F(mmt_iounet_head, c4);
      F(mmt_iounet_head, n3); F(mmt_iounet_head, n4);
      break;
    case 14:
      v.push_back(sizeof(mmt_iounet_map));
      F(mmt_iounet_map, p); F(mmt_iounet_map, H); F(mmt_iounet_map, W); F(mmt_iounet_map, pix);
      F(mmt_iounet_map, row); F(mmt_iounet_map, img);
      break;
    case 15:
      v.push_back(sizeof(mmt_iounet_feat));
      F(mmt_iounet_feat, B); F(mmt_iounet_feat, pad_); F(mmt_iounet_feat, l3); F(mmt_iounet_feat, l4);
      break;
    default:
      return 0;
  }
#undef F
  for (int i = 0; i < (int)v.size() && i < cap && out; ++i) out[i] = v[i];
  return (int)v.size();
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

// ---- SiamFC pool (siamfc_pool.hip): every argument is checked before any HIP call
int mmt_siamfc_pool_crop(const mmt_siamfc_state* states, const mmt_dimp_frame* frames, int n,
                         const mmt_siamfc_params* params, float* out, int* windows, void* stream) {
  if (!states || !frames || !out || !siamfc_params_ok(params, n)) return MMT_E_ARG;
  siamfc_pool_crop(reinterpret_cast<const SiamState*>(states), reinterpret_cast<const SiamFrame*>(frames), n,
                   *reinterpret_cast<const SiamParams*>(params), out, windows, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_xcorr_nhwc_group(const float* z, int64_t z_bstride, int group, const float* x, float* out, int B, int Cc,
                         int hz, int wz, int hx, int wx, float scale, float bias, void* stream) {
  if (!z || !x || !out || B <= 0 || group < 1 || Cc <= 0 || hz <= 0 || wz <= 0 || hx < hz || wx < wz || z_bstride < 0 ||
      (int64_t)hz * wz * Cc > 16384 || B > 65535 ||
      ((Cc & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z) | (uintptr_t)z_bstride * 4) & 15)))
    return MMT_E_ARG;
  xcorr_nhwc_group(z, z_bstride, group, x, out, B, Cc, hz, wz, hx, wx, scale, bias, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_siamfc_pool_update(const float* resp, int n, const mmt_siamfc_params* params, const double* hann1d,
                           float* scratch, mmt_siamfc_state* states, mmt_siamfc_result* results,
                           mmt_siamfc_result* host_results, void* stream) {
  if (!resp || !hann1d || !scratch || !states || !results || !siamfc_params_ok(params, n)) return MMT_E_ARG;
  siamfc_pool_update(resp, n, *reinterpret_cast<const SiamParams*>(params), hann1d, scratch,
                     reinterpret_cast<SiamState*>(states), reinterpret_cast<SiamResult*>(results),
                     reinterpret_cast<SiamResult*>(host_results), (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int mmt_op_gemm(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* Cp, int64_t ldc,
                const float* R, int64_t ldr, int M, int N, int K, int epi, int conv_hw, int conv_cin, int pos_rows,
                void* stream) {
  if (!A || !W || !Cp || M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 32 || epi < 0 || epi > 6) return MMT_E_ARG;
  if ((epi == EPI_RESID_F32 || epi == EPI_POS_F32) && !R) return MMT_E_ARG;
  if (conv_hw > 0 && (conv_cin % 64 || K != 9 * conv_cin || (epi != EPI_RELU_BF16 && epi != EPI_RELU_F32)))
    return MMT_E_ARG;
  float* ws = op_workspace();
  GemmArgs a{};
  a.g[0] = GemmGroup{(const bf16_t*)A, nullptr, lda, (const bf16_t*)W, nullptr, ldw, bias, Cp, nullptr, ldc, R, ldr};
  a.groups = 1;
  a.zero = op_zero_page();
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

int mmt_op_gemm_ex(const mmt_gemm_ex_args* x, mmt_gemm_ran* ran, void* stream) {
  if (!x || x->groups < 1 || x->groups > 3 || x->M <= 0 || x->N <= 0 || x->K <= 0 || x->K % 64 || x->N % 32 ||
      x->epi < 0 || x->epi > 6 || x->ws_elems < 0 || (x->ws_elems > 0 && !x->ws))
    return MMT_E_ARG;
  const int epi = x->epi;
  const bool out16 = epi == EPI_BF16 || epi == EPI_GELU_BF16 || epi == EPI_RELU_BF16;
  const bool has_r = epi == EPI_RESID_F32 || epi == EPI_POS_F32;
  const bool conv = x->conv_hw > 0;
  if (conv && (x->conv_cin <= 0 || x->conv_cin % 64 || x->K != 9 * x->conv_cin ||
               (epi != EPI_RELU_BF16 && epi != EPI_RELU_F32)))
    return MMT_E_ARG;
  GemmArgs a{};
  for (int i = 0; i < x->groups; ++i) {
    const mmt_gemm_group& g = x->g[i];
    if (!g.A || !g.W || !g.C || (x->split && (!g.A_lo || !g.W_lo || (out16 && !g.C_lo))) || (has_r && !g.R) ||
        (conv && g.lda < x->conv_cin))
      return MMT_E_ARG;
    a.g[i] = GemmGroup{(const bf16_t*)g.A, (const bf16_t*)g.A_lo, g.lda, (const bf16_t*)g.W, (const bf16_t*)g.W_lo,
                       g.ldw, g.bias, g.C, g.C_lo, g.ldc, g.R, g.ldr, g.inv, g.out_scale};
  }
  a.groups = x->groups;
  a.M = x->M;
  a.N = x->N;
  a.K = x->K;
  a.amode = conv ? A_CONV3 : A_DENSE;
  a.conv_hw = x->conv_hw;
  a.conv_cin = x->conv_cin;
  a.pos_rows = x->pos_rows > 0 ? x->pos_rows : 1;
  a.split = x->split ? 1 : 0;
  a.ws = x->ws_elems > 0 ? x->ws : nullptr;
  a.ws_elems = x->ws_elems;
  a.zero = a.split ? nullptr : op_zero_page();
  a.defer_reduce = x->defer_reduce ? 1 : 0;
  a.conc = x->conc;
  const GemmPlan p = gemm_plan_of(a, epi);   // the plan gemm() launches below
  if (gemm(a, epi, (hipStream_t)stream) < 0) return MMT_E_ARG;   // no kernel for this shape / epilogue: nothing ran
  if (ran) {
    snprintf(ran->tile, sizeof ran->tile, "%s", gemm_tile_name(p.tile));
    ran->ksplit = p.ksplit;
    ran->deferred = p.defer ? 1 : 0;
  }
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
  a.qk_inv = 0.125f / (s_qkv * s_qkv);   // the engine's arguments (engine_forward.cpp block), head dim 64
  a.pv_inv = 1.0f / (16384.0f * s_qkv);
  a.out_scale = s_qkv;
  attention(a, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

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
  } else {       // the engine's two-launch branch (engine_forward.cpp block)
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
