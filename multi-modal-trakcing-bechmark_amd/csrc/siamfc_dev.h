// Device code shared by the sequential SiamFC kernels (siamfc.hip, imaging.hip) and the pooled ones
// (siamfc_pool.hip): the pooled kernels must give the sequential kernels' bits, so both call the functions below
// instead of restating them.
//  * xcorr_nhwc_pixel: one wave's NHWC correlation sum of one output pixel (lanes over channels, fixed butterfly);
//  * siamfc_response_select: the post-correlation selection of TrackerSiamFC.update for one sequence, by one
//    1 024-thread workgroup.
#pragma once
#include "cvresize.h"
#include "kernels.h"

namespace mmt {

// sum_{i,j,c} xb[(y+i)][(x+j)][c] * zsh[i][j][c] of one wave: lanes over channels (float4 when C % 4 == 0), the
// partial sums combined in a fixed butterfly order (every lane returns the total)
__device__ __forceinline__ float xcorr_nhwc_pixel(const float* __restrict__ xb, const float* zsh, int C, int hz, int wz,
                                                  int wx, int y, int x, int lane) {
  float acc = 0.f;
  if ((C & 3) == 0) {
    const int c4 = C >> 2;
    for (int i = 0; i < hz; ++i)
      for (int j = 0; j < wz; ++j) {
        const float4* xr = reinterpret_cast<const float4*>(xb + ((int64_t)(y + i) * wx + x + j) * C);
        const float4* zr = reinterpret_cast<const float4*>(zsh + (i * wz + j) * C);
        for (int c = lane; c < c4; c += 64) {
          const float4 u = xr[c], v = zr[c];
          acc += u.x * v.x + u.y * v.y + u.z * v.z + u.w * v.w;
        }
      }
  } else {
    for (int i = 0; i < hz; ++i)
      for (int j = 0; j < wz; ++j) {
        const float* xr = xb + ((int64_t)(y + i) * wx + x + j) * C;
        const float* zr = zsh + (i * wz + j) * C;
        for (int c = lane; c < C; c += 64) acc += xr[c] * zr[c];
      }
  }
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  return acc;
}

constexpr int RT = 1024;   // threads of a response workgroup

__device__ __forceinline__ float block_reduce_f(float v, float* red, bool is_max, bool is_min) {
  const int t = threadIdx.x;
  for (int o = 32; o >= 1; o >>= 1) {
    const float u = __shfl_xor(v, o, 64);
    v = is_max ? fmaxf(v, u) : (is_min ? fminf(v, u) : v + u);
  }
  __syncthreads();
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  if (t < 64) {
    v = t < RT / 64 ? red[t] : (is_max ? -INFINITY : (is_min ? INFINITY : 0.f));
    for (int o = 32; o >= 1; o >>= 1) {
      const float u = __shfl_xor(v, o, 64);
      v = is_max ? fmaxf(v, u) : (is_min ? fminf(v, u) : v + u);
    }
    if (t == 0) red[RT / 64] = v;
  }
  __syncthreads();
  return red[RT / 64];
}

// a.resp / a.scratch of one sequence -> scale id, flat index into the up x up map and the windowed maximum, valid
// in thread 0 (a.result is not used); called by all RT threads of the workgroup
__device__ __forceinline__ void siamfc_response_select(const SiamRespArgs& a, int& out_sid, int& out_idx,
                                                       double& out_val) {
#pragma clang fp contract(off)   // numpy's separate float32 / float64 roundings
  __shared__ float red[RT / 64 + 1];
  __shared__ double dv[RT];
  __shared__ int di[RT];
  __shared__ float smax[8];
  const int t = threadIdx.x, U = a.up, UU = U * U, mid = a.n / 2;
  // 1. upsample every scale, penalise the off-centre scales, per-scale max
  for (int s = 0; s < a.n; ++s) {
    const float* src = a.resp + (int64_t)s * a.r * a.r;
    float* dst = a.scratch + (int64_t)s * UU;
    float m = -INFINITY;
    for (int i = t; i < UU; i += RT) {
      const int oy = i / U, ox = i - oy * U;
      float v = cv_cubic_f32(src, a.r, U, oy, ox);
      if (s != mid) v = __fmul_rn(v, a.penalty);
      dst[i] = v;
      m = fmaxf(m, v);
    }
    m = block_reduce_f(m, red, true, false);
    if (t == 0) smax[s] = m;
  }
  __syncthreads();
  int sid = 0;
  for (int s = 1; s < a.n; ++s)
    if (smax[s] > smax[sid]) sid = s;
  const float* r = a.scratch + (int64_t)sid * UU;
  // 2. response -= min; response /= sum + 1e-16
  float mn = INFINITY;
  for (int i = t; i < UU; i += RT) mn = fminf(mn, r[i]);
  mn = block_reduce_f(mn, red, false, true);
  float sm = 0.f;
  for (int i = t; i < UU; i += RT) sm += __fsub_rn(r[i], mn);
  sm = block_reduce_f(sm, red, false, false);
  const float div = (float)((double)sm + 1e-16);
  // 3. (1 - wi) * response + wi * hann (double), first-occurrence argmax
  double best = -1e300;
  int bi = 0x7fffffff;
  for (int i = t; i < UU; i += RT) {
    const int y = i / U, x = i - y * U;
    const float nv = __fdiv_rn(__fsub_rn(r[i], mn), div);
    const double v = (double)__fmul_rn(a.one_minus_wi, nv) + a.wi * ((a.hann1d[y] * a.hann1d[x]) / a.hann_sum);
    if (v > best) { best = v; bi = i; }
  }
  dv[t] = best;
  di[t] = bi;
  __syncthreads();
  for (int st = RT / 2; st > 0; st >>= 1) {
    if (t < st) {
      const double v2 = dv[t + st];
      const int i2 = di[t + st];
      if (v2 > dv[t] || (v2 == dv[t] && i2 < di[t])) { dv[t] = v2; di[t] = i2; }
    }
    __syncthreads();
  }
  out_sid = sid;
  out_idx = di[0];
  out_val = dv[0];
}

}  // namespace mmt
