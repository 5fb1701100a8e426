// IoU-Net's predictor head and box ascent on gfx950 (ltr/models/bbreg/atom_iou_net.py:96-136 and
// pytracking/tracker/dimp/dimp.py:727-752, restated): fp32 throughout, the products on v_mfma_f32_16x16x4_f32 (the
// box gradient is what the ascent follows, so no reduced-precision products).  Pooling and its box gradient are
// prroi.hip's entries, called as any caller does; the per-box arithmetic and the K split are iounet_dev.h's.
//
//   iou_linear_partial_kernel  X[R][Kd] . W[N][Kd]^T over one slice of kIouSlice columns of Kd: grid (N / 64, slices,
//                              R / 16); the four waves of a workgroup take a quarter of the slice each and a 16 x 64
//                              tile of outputs; a lane loads 16 bytes of a row of X and of four rows of W per step and
//                              feeds the four values to four MFMAs, so the order of a row's sum is fixed by Kd alone.
//                              X is scaled on load by the modulation (row r: sequence r / P, column k: channel k / bins).
//                              The waves' tiles meet in LDS and leave as one partial tile, added in wave order.
//   iou_linear_reduce_kernel   Y = act(sum of the slices in slice order + b)
//   iou_head_kernel            one workgroup per row: both hidden layers' slices summed in slice order, bias, ReLU,
//                              iou = w_p . [h3, h4] + b_p (a lane over its columns in order, the 64 lanes by an xor
//                              butterfly, the waves through LDS in wave order) and g_h = grad_iou * w_p * (h > 0)
//   iou_linear_t_kernel        G[R][Kd] = g_h[R][N] . W[N][Kd], times the modulation: grid (Kd / 64, R / 16); the four
//                              waves split N and meet in LDS as above; G is [K][C][PH][PW], PrRoIPool's grad_out
//   iou_rois_kernel, iou_box_kernel   one thread per box, iounet_dev.h's arithmetic
// No atomics, no scratch, every output element written by one thread in a fixed order: two runs give the same bits,
// and a row's results do not depend on which other rows are in the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmtrack.h"
#include "iounet_dev.h"

namespace mmt {

typedef float iou_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIouThreads = 256;          // four waves
constexpr int kIouRows = 16, kIouCols = 64;   // a workgroup's output tile
constexpr int kIouPool3 = 5, kIouPool4 = 3;   // PrRoIPool2D(5, 5, 1/8) and (3, 3, 1/16) of the reference
constexpr float kIouScale3 = 1.f / 8.f, kIouScale4 = 1.f / 16.f;

// the waves' 16 x 64 accumulator tiles -> LDS [wave][row][col]; accumulator j of lane column c is tile column 16 j + c, or
// 4 c + j when the lane's four accumulators are four consecutive columns (the transposed kernel)
template <bool kInterleaved>
__device__ __forceinline__ void iou_stage_tiles(float (*red)[kIouRows * kIouCols], const iou_f32x4* acc, int wave, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      red[wave][(4 * g + i) * kIouCols + (kInterleaved ? 4 * c + j : 16 * j + c)] = acc[j][i];
}

__global__ __launch_bounds__(kIouThreads) void iou_linear_partial_kernel(const float* __restrict__ X, int R, int Kd,
                                                                         const float* __restrict__ W, int N,
                                                                         const float* __restrict__ scale, int P, int bins,
                                                                         float* __restrict__ part) {
  __shared__ float red[4][kIouRows * kIouCols];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kIouCols, s = blockIdx.y, r0 = blockIdx.z * kIouRows;
  const int row = r0 + c;
  const bool row_ok = row < R;
  const int C = scale ? Kd / bins : 0;
  const float* xr = X + (int64_t)(row_ok ? row : 0) * Kd;
  const float* mr = scale ? scale + (int64_t)((row_ok ? row : 0) / P) * C : nullptr;
  iou_f32x4 acc[4] = {};
  const int kw = s * kIouSlice + wave * (kIouSlice / 4);
#pragma unroll
  for (int step = 0; step < kIouSlice / 64; ++step) {
    const int k = kw + step * 16 + 4 * g;
    const bool k_ok = k < Kd;   // Kd % 4 == 0: the four columns are in or out together
    // every lane loads from a clamped, valid address and zeroes what is out of range afterwards: an MFMA reads the
    // registers of all 64 lanes whatever the execution mask, so no operand may be left unloaded on a skipped branch
    const int kl = k_ok ? k : Kd - 4;
    float4 x = *reinterpret_cast<const float4*>(xr + kl);
    if (scale) {
      const unsigned ub = bins;
      x.x *= mr[(unsigned)kl / ub];
      x.y *= mr[(unsigned)(kl + 1) / ub];
      x.z *= mr[(unsigned)(kl + 2) / ub];
      x.w *= mr[(unsigned)(kl + 3) / ub];
    }
    const float xs = (row_ok && k_ok) ? 1.f : 0.f;
    x.x = xs != 0.f ? x.x : 0.f;
    x.y = xs != 0.f ? x.y : 0.f;
    x.z = xs != 0.f ? x.z : 0.f;
    x.w = xs != 0.f ? x.w : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 16 * j + c;
      float4 w = *reinterpret_cast<const float4*>(W + (int64_t)(n < N ? n : N - 1) * Kd + kl);
      const bool w_ok = n < N && k_ok;
      w.x = w_ok ? w.x : 0.f;
      w.y = w_ok ? w.y : 0.f;
      w.z = w_ok ? w.z : 0.f;
      w.w = w_ok ? w.w : 0.f;
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, w.x, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, w.y, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, w.z, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, w.w, acc[j], 0, 0, 0);
    }
  }
  iou_stage_tiles<false>(red, acc, wave, lane);
  __syncthreads();
  for (int e = threadIdx.x; e < kIouRows * kIouCols; e += kIouThreads) {
    const int r = r0 + e / kIouCols, n = n0 + e % kIouCols;
    if (r < R && n < N) part[((int64_t)s * R + r) * N + n] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  }
}

__global__ __launch_bounds__(kIouThreads) void iou_linear_reduce_kernel(const float* __restrict__ part, int S, int R, int N,
                                                                        const float* __restrict__ bias, int relu,
                                                                        float* __restrict__ Y) {
  const int64_t i = (int64_t)blockIdx.x * kIouThreads + threadIdx.x, RN = (int64_t)R * N;
  if (i >= RN) return;
  float v = part[i];
  for (int s = 1; s < S; ++s) v += part[s * RN + i];
  if (bias) v += bias[i % N];
  Y[i] = relu ? fmaxf(v, 0.f) : v;
}

struct IouHead {
  const float *part3, *part4, *b3, *b4, *wp;
  float bp;
  int S3, S4, N3, N4, R;
};

__global__ __launch_bounds__(kIouThreads) void iou_head_kernel(IouHead h, const float* __restrict__ grad_iou,
                                                               float* __restrict__ iou, float* __restrict__ gh3,
                                                               float* __restrict__ gh4) {
  __shared__ float red[kIouThreads / 64];
  const int r = blockIdx.x;
  const float gi = grad_iou ? grad_iou[r] : 1.f;
  float dot = 0.f;
  for (int n = threadIdx.x; n < h.N3 + h.N4; n += kIouThreads) {
    const bool l3 = n < h.N3;
    const int m = l3 ? n : n - h.N3, N = l3 ? h.N3 : h.N4, S = l3 ? h.S3 : h.S4;
    const float* p = (l3 ? h.part3 : h.part4) + (int64_t)r * N + m;
    const int64_t RN = (int64_t)h.R * N;
    float v = p[0];
    for (int s = 1; s < S; ++s) v += p[s * RN];
    v += (l3 ? h.b3 : h.b4)[m];
    const float w = h.wp[n], a = fmaxf(v, 0.f);
    dot += w * a;
    (l3 ? gh3 : gh4)[(int64_t)r * N + m] = v > 0.f ? gi * w : 0.f;
  }
  for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
  __syncthreads();
  if (threadIdx.x == 0) iou[r] = (((red[0] + red[1]) + red[2]) + red[3]) + h.bp;
}

__global__ __launch_bounds__(kIouThreads) void iou_linear_t_kernel(const float* __restrict__ gh, int R, int N,
                                                                   const float* __restrict__ W, int Kd,
                                                                   const float* __restrict__ scale, int P, int bins,
                                                                   float* __restrict__ G) {
  __shared__ float red[4][kIouRows * kIouCols];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), c = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * kIouCols, r0 = blockIdx.y * kIouRows;
  const int row = r0 + c, kc = k0 + 4 * c;
  const bool row_ok = row < R, k_ok = kc < Kd;
  const int kl = k_ok ? kc : Kd - 4;
  const float* gr = gh + (int64_t)(row_ok ? row : 0) * N;
  iou_f32x4 acc[4] = {};
  for (int nn = wave * 16; nn < N; nn += 64) {   // N % 16 == 0
    const int n = nn + 4 * g;
    float4 a = *reinterpret_cast<const float4*>(gr + n);   // clamped addresses, zeroed after the load (see above)
    a.x = row_ok ? a.x : 0.f;
    a.y = row_ok ? a.y : 0.f;
    a.z = row_ok ? a.z : 0.f;
    a.w = row_ok ? a.w : 0.f;
    const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float4 w = *reinterpret_cast<const float4*>(W + (int64_t)(n + t) * Kd + kl);
      w.x = k_ok ? w.x : 0.f;
      w.y = k_ok ? w.y : 0.f;
      w.z = k_ok ? w.z : 0.f;
      w.w = k_ok ? w.w : 0.f;
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], w.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], w.y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], w.z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], w.w, acc[3], 0, 0, 0);
    }
  }
  iou_stage_tiles<true>(red, acc, wave, lane);
  __syncthreads();
  const int C = scale ? Kd / bins : 0;
  for (int e = threadIdx.x; e < kIouRows * kIouCols; e += kIouThreads) {
    const int r = r0 + e / kIouCols, k = k0 + e % kIouCols;
    if (r < R && k < Kd) {
      float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
      if (scale) v *= scale[(int64_t)(r / P) * C + k / bins];
      G[(int64_t)r * Kd + k] = v;
    }
  }
}

__global__ __launch_bounds__(kIouThreads) void iou_rois_kernel(const float* __restrict__ boxes, int R, int P,
                                                               float* __restrict__ rois) {
  const int r = blockIdx.x * kIouThreads + threadIdx.x;
  if (r >= R) return;
  const float b[4] = {boxes[4 * r], boxes[4 * r + 1], boxes[4 * r + 2], boxes[4 * r + 3]};
  float o[5];
  iou_box_to_roi(b, r / P, o);
  for (int j = 0; j < 5; ++j) rois[5 * r + j] = o[j];
}

// step == nullptr: write the box gradient to out; otherwise out = box + step * grad * (w, h, w, h)
__global__ __launch_bounds__(kIouThreads) void iou_box_kernel(const float* __restrict__ groi3, const float* __restrict__ groi4,
                                                              int R, const float* boxes, float step_pos, float step_size,
                                                              float* out) {
  const int r = blockIdx.x * kIouThreads + threadIdx.x;
  if (r >= R) return;
  float g3[5], g4[5], gb[4], o[4];
  for (int j = 0; j < 5; ++j) {
    g3[j] = groi3[5 * r + j];
    g4[j] = groi4[5 * r + j];
  }
  iou_fold_grad(g3, g4, gb);
  if (boxes) {
    const float b[4] = {boxes[4 * r], boxes[4 * r + 1], boxes[4 * r + 2], boxes[4 * r + 3]};
    iou_step(b, gb, step_pos, step_size, o);
  } else {
    for (int j = 0; j < 4; ++j) o[j] = gb[j];
  }
  *reinterpret_cast<float4*>(out + 4 * r) = make_float4(o[0], o[1], o[2], o[3]);
}

static inline int iou_last_err() { return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP; }
static inline bool iou_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline bool iou_finite(float v) { return v - v == 0.f; }

constexpr int kIouMaxRows = 1 << 19;   // keeps every grid dimension and 5 * R in range

static bool iou_bad_linear(int R, int Kd, int N) {
  return R < 1 || R > kIouMaxRows || Kd < 4 || Kd % 4 || N < 1 || Kd > (1 << 24) || N > (1 << 20) ||
         iou_ksplit(Kd) > 65535;
}

static bool iou_bad_head_shape(int c3, int c4, int n3, int n4) {
  return c3 < 4 || c4 < 4 || c3 % 4 || c4 % 4 || n3 < 16 || n4 < 16 || n3 % 16 || n4 % 16 || c3 > (1 << 16) ||
         c4 > (1 << 16) || n3 > (1 << 16) || n4 > (1 << 16);
}

// the predictor's workspace, in floats from its start; every part is a multiple of 4 floats
struct IouWs {
  int64_t rois, pool3, pool4, part3, part4, gh3, gh4, G3, G4, groi3, groi4, total;
};
static IouWs iou_ws(int64_t R, int64_t kd3, int64_t kd4, int64_t n3, int64_t n4) {
  IouWs w;
  int64_t o = 0;
  auto take = [&](int64_t n) { const int64_t at = o; o += n; return at; };
  w.rois = take(8 * R);
  w.pool3 = take(R * kd3);
  w.pool4 = take(R * kd4);
  w.part3 = take(iou_ksplit((int)kd3) * R * n3);
  w.part4 = take(iou_ksplit((int)kd4) * R * n4);
  w.gh3 = take(R * n3);
  w.gh4 = take(R * n4);
  w.G3 = take(R * kd3);
  w.G4 = take(R * kd4);
  w.groi3 = take(8 * R);
  w.groi4 = take(8 * R);
  w.total = o;
  return w;
}

static int iou_linear_partial(const float* X, int R, int Kd, const float* W, int N, const float* scale, int P, int bins,
                              float* part, hipStream_t st) {
  const dim3 grid((N + kIouCols - 1) / kIouCols, iou_ksplit(Kd), (R + kIouRows - 1) / kIouRows);
  hipLaunchKernelGGL(iou_linear_partial_kernel, grid, dim3(kIouThreads), 0, st, X, R, Kd, W, N, scale, P, bins, part);
  return iou_last_err();
}

static int iou_linear_t(const float* gh, int R, int N, const float* W, int Kd, const float* scale, int P, int bins,
                        float* G, hipStream_t st) {
  const dim3 grid((Kd + kIouCols - 1) / kIouCols, (R + kIouRows - 1) / kIouRows);
  hipLaunchKernelGGL(iou_linear_t_kernel, grid, dim3(kIouThreads), 0, st, gh, R, N, W, Kd, scale, P, bins, G);
  return iou_last_err();
}

static bool iou_bad_map(const mmt_iounet_map& m, int C) {
  if (!m.p || iou_misaligned(m.p) || m.H < 1 || m.W < 1 || m.pix < C || m.pix % 4 || m.row % 4 || m.img % 4) return true;
  const int64_t row_extent = (int64_t)(m.W - 1) * m.pix + C;
  return m.row < row_extent || m.img < (int64_t)(m.H - 1) * m.row + row_extent;
}

// every check of predict and refine (no HIP call)
static bool iou_bad_call(const mmt_iounet_head* h, const mmt_iounet_feat* f, const float* mod3, const float* mod4,
                         const float* boxes, int P, const void* ws, size_t ws_bytes) {
  if (!h || !f || !mod3 || !mod4 || !boxes || !ws || iou_misaligned(ws) || iou_misaligned(boxes)) return true;
  if (!h->w3 || !h->b3 || !h->w4 || !h->b4 || !h->wp || iou_misaligned(h->w3) || iou_misaligned(h->w4) ||
      !iou_finite(h->bp) || iou_bad_head_shape(h->c3, h->c4, h->n3, h->n4))
    return true;
  if (f->B < 1 || P < 1 || (int64_t)f->B * P > kIouMaxRows || iou_bad_map(f->l3, h->c3) || iou_bad_map(f->l4, h->c4))
    return true;
  const IouWs w = iou_ws((int64_t)f->B * P, (int64_t)h->c3 * kIouPool3 * kIouPool3, (int64_t)h->c4 * kIouPool4 * kIouPool4,
                         h->n3, h->n4);
  return ws_bytes < (size_t)w.total * 4;
}

// one forward of the boxes at `boxes` (and, with gbox or step_boxes, the box gradient: written to gbox, or applied as
// one ascent step to step_boxes in place)
static int iou_pass(const mmt_iounet_head* h, const mmt_iounet_feat* f, const float* mod3, const float* mod4,
                    const float* boxes, int P, const float* grad_iou, float* iou, float* gbox, float* step_boxes,
                    float step_pos, float step_size, float* ws, hipStream_t st) {
  const int B = f->B, R = B * P, b3 = kIouPool3 * kIouPool3, b4 = kIouPool4 * kIouPool4;
  const int kd3 = h->c3 * b3, kd4 = h->c4 * b4;
  const IouWs w = iou_ws(R, kd3, kd4, h->n3, h->n4);
  const int blocks = (R + kIouThreads - 1) / kIouThreads;
  int rc;
  hipLaunchKernelGGL(iou_rois_kernel, dim3(blocks), dim3(kIouThreads), 0, st, boxes, R, P, ws + w.rois);
  if ((rc = iou_last_err()) != MMT_OK) return rc;
  if ((rc = mmt_prroi_pool_rois(f->l3.p, B, f->l3.H, f->l3.W, h->c3, f->l3.pix, f->l3.row, f->l3.img, ws + w.rois, R,
                                kIouScale3, kIouPool3, kIouPool3, ws + w.pool3, st)) != MMT_OK)
    return rc;
  if ((rc = mmt_prroi_pool_rois(f->l4.p, B, f->l4.H, f->l4.W, h->c4, f->l4.pix, f->l4.row, f->l4.img, ws + w.rois, R,
                                kIouScale4, kIouPool4, kIouPool4, ws + w.pool4, st)) != MMT_OK)
    return rc;
  if ((rc = iou_linear_partial(ws + w.pool3, R, kd3, h->w3, h->n3, mod3, P, b3, ws + w.part3, st)) != MMT_OK) return rc;
  if ((rc = iou_linear_partial(ws + w.pool4, R, kd4, h->w4, h->n4, mod4, P, b4, ws + w.part4, st)) != MMT_OK) return rc;
  const IouHead hd{ws + w.part3, ws + w.part4, h->b3, h->b4, h->wp, h->bp, iou_ksplit(kd3), iou_ksplit(kd4), h->n3, h->n4, R};
  hipLaunchKernelGGL(iou_head_kernel, dim3(R), dim3(kIouThreads), 0, st, hd, grad_iou, iou, ws + w.gh3, ws + w.gh4);
  if ((rc = iou_last_err()) != MMT_OK) return rc;
  if (!gbox && !step_boxes) return MMT_OK;
  if ((rc = iou_linear_t(ws + w.gh3, R, h->n3, h->w3, kd3, mod3, P, b3, ws + w.G3, st)) != MMT_OK) return rc;
  if ((rc = iou_linear_t(ws + w.gh4, R, h->n4, h->w4, kd4, mod4, P, b4, ws + w.G4, st)) != MMT_OK) return rc;
  if ((rc = mmt_prroi_pool_rois_grad_rois(f->l3.p, B, f->l3.H, f->l3.W, h->c3, f->l3.pix, f->l3.row, f->l3.img,
                                          ws + w.rois, R, kIouScale3, kIouPool3, kIouPool3, ws + w.pool3, ws + w.G3,
                                          ws + w.groi3, st)) != MMT_OK)
    return rc;
  if ((rc = mmt_prroi_pool_rois_grad_rois(f->l4.p, B, f->l4.H, f->l4.W, h->c4, f->l4.pix, f->l4.row, f->l4.img,
                                          ws + w.rois, R, kIouScale4, kIouPool4, kIouPool4, ws + w.pool4, ws + w.G4,
                                          ws + w.groi4, st)) != MMT_OK)
    return rc;
  hipLaunchKernelGGL(iou_box_kernel, dim3(blocks), dim3(kIouThreads), 0, st, ws + w.groi3, ws + w.groi4, R,
                     step_boxes, step_pos, step_size, step_boxes ? step_boxes : gbox);
  return iou_last_err();
}

}  // namespace mmt

using namespace mmt;

extern "C" {

size_t mmt_iounet_linear_ws_bytes(int rows, int Kd, int N) {
  if (iou_bad_linear(rows, Kd, N)) return 0;
  return (size_t)iou_ksplit(Kd) * rows * N * 4;
}

size_t mmt_iounet_ws_bytes(int rows, int Kd3, int Kd4, int N3, int N4) {
  if (rows < 1 || rows > kIouMaxRows || Kd3 < 1 || Kd4 < 1 || Kd3 % (kIouPool3 * kIouPool3) || Kd4 % (kIouPool4 * kIouPool4) ||
      iou_bad_head_shape(Kd3 / (kIouPool3 * kIouPool3), Kd4 / (kIouPool4 * kIouPool4), N3, N4))
    return 0;
  return (size_t)iou_ws(rows, Kd3, Kd4, N3, N4).total * 4;
}

int mmt_iounet_linear(const float* X, int rows, int Kd, const float* W, int N, const float* bias, const float* scale,
                      int rows_per_group, int bins, int relu, float* Y, void* ws, size_t ws_bytes, void* stream) {
  if (!X || !W || !Y || !ws || iou_bad_linear(rows, Kd, N) || iou_misaligned(X) || iou_misaligned(W) || iou_misaligned(ws) ||
      ws_bytes < (size_t)iou_ksplit(Kd) * rows * N * 4)
    return MMT_E_ARG;
  if (scale && (rows_per_group < 1 || bins < 1 || Kd % bins)) return MMT_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = iou_linear_partial(X, rows, Kd, W, N, scale, rows_per_group, bins, (float*)ws, st)) != MMT_OK) return rc;
  const int64_t items = (int64_t)rows * N;
  hipLaunchKernelGGL(iou_linear_reduce_kernel, dim3((unsigned)((items + kIouThreads - 1) / kIouThreads)), dim3(kIouThreads), 0,
                     st, (const float*)ws, iou_ksplit(Kd), rows, N, bias, relu, Y);
  return iou_last_err();
}

int mmt_iounet_predict(const mmt_iounet_head* head, const mmt_iounet_feat* feat, const float* mod3, const float* mod4,
                       const float* boxes, int P, const float* grad_iou, float* iou, float* grad_boxes, void* ws,
                       size_t ws_bytes, void* stream) {
  if (!iou || iou_bad_call(head, feat, mod3, mod4, boxes, P, ws, ws_bytes) || (grad_boxes && iou_misaligned(grad_boxes)))
    return MMT_E_ARG;
  return iou_pass(head, feat, mod3, mod4, boxes, P, grad_iou, iou, grad_boxes, nullptr, 0.f, 0.f, (float*)ws,
                  (hipStream_t)stream);
}

int mmt_iounet_refine(const mmt_iounet_head* head, const mmt_iounet_feat* feat, const float* mod3, const float* mod4,
                      const float* boxes, int P, int iters, float step_pos, float step_size, float step_decay,
                      float* boxes_out, float* iou, void* ws, size_t ws_bytes, void* stream) {
  if (!iou || !boxes_out || iou_misaligned(boxes_out) || iters < 1 || iters > 1024 || !iou_finite(step_pos) ||
      !iou_finite(step_size) || !iou_finite(step_decay) || iou_bad_call(head, feat, mod3, mod4, boxes, P, ws, ws_bytes))
    return MMT_E_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const int R = feat->B * P;
  if (boxes_out != boxes &&
      hipMemcpyAsync(boxes_out, boxes, (size_t)R * 16, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return MMT_E_HIP;
  for (int it = 0; it < iters; ++it) {
    const int rc = iou_pass(head, feat, mod3, mod4, boxes_out, P, nullptr, iou, nullptr, boxes_out, step_pos, step_size,
                            (float*)ws, st);
    if (rc != MMT_OK) return rc;
    step_pos = iou_mul(step_pos, step_decay);
    step_size = iou_mul(step_size, step_decay);
  }
  return MMT_OK;
}

}  // extern "C"
