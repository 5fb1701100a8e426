// Precise RoI Pooling over any ROI list on gfx950 (fp32): forward, gradient to the box coordinates and gradient to
// the feature map (ltr/external/PreciseRoIPooling, its three kernels restated; the arithmetic is prroi_dev.h's, whose
// header states the robustness contract).  The feature map is channels-last with the channel stride 1 and the pixel,
// row and image pitches given in floats; rois is a device list [K][5] = batch index, x0, y0, x1, y1.
//
//   prroi_fwd_kernel        grid (K, channel chunks): a workgroup owns one ROI's bins for a chunk of channels; a work item
//                           is (bin, 4 channels) with the channel vector fastest, so a wave's lanes read consecutive
//                           16-byte pieces of a pixel; results are staged in LDS as [c][bin] and leave as full lines
//   prroi_grad_roi_kernel   one workgroup per ROI; fixed reduction order: a lane over its items in index order, the
//                           64 lanes by an xor butterfly, the 16 waves through LDS in wave order; thread 0 writes the
//                           five values (no atomics, no pre-zeroed output)
//   prroi_grad_feat_kernel  gather: a thread owns (pixel, 4 channels) of image n, walks the ROI list in order and
//                           adds coefficient * grad_out / area of every bin that touches its pixel; every element of
//                           grad_feat is written
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmtrack.h"
#include "prroi_dev.h"

namespace mmt {

constexpr int kPrThreads = 256;
constexpr int kPrGradThreads = 1024;   // the box gradient's workgroup: one per ROI, so a large one
constexpr int kPrStage = 8192;   // floats of the forward's LDS stage (32 KiB): a chunk of channels x PH x PW bins

struct PrFeat {
  const float* p;
  int64_t pix, row, img;   // pitches in floats
  int N, H, W, C;
};

struct PrGet4 {
  const float* base;   // image n, channel c0
  int64_t pix, row;
  __device__ __forceinline__ PrV4 operator()(int h, int w) const {
    const float4 v = *reinterpret_cast<const float4*>(base + h * row + w * pix);
    return PrV4{v.x, v.y, v.z, v.w};
  }
};

// channels of one forward workgroup: all of them when they fit the stage, otherwise the largest multiple of 4 that
// does (PH * PW <= 64, so at least 128); halved, down to 64 at the least, while the grid has fewer than 1 024
// workgroups (a short ROI list would otherwise leave most of the chip idle)
static inline int prroi_chunk(int C, int PH, int PW, int K) {
  const int fit = (kPrStage / (PH * PW)) & ~3;
  int chunk = C < fit ? C : fit;
  while (chunk > 64 && chunk % 8 == 0 && (int64_t)K * ((C + chunk - 1) / chunk) < 1024) chunk /= 2;
  return chunk;
}

__global__ __launch_bounds__(kPrThreads) void prroi_fwd_kernel(PrFeat f, const float* __restrict__ rois, float scale,
                                                               int PH, int PW, int chunk, float* __restrict__ out) {
  __shared__ float stage[kPrStage];
  const int k = blockIdx.x, c0 = blockIdx.y * chunk, bins = PH * PW;
  const int nc = min(chunk, f.C - c0), nc4 = nc >> 2;
  const PrRoi roi = prroi_roi(rois + (int64_t)k * 5, f.N, scale, PH, PW);
  for (int it = threadIdx.x; it < bins * nc4; it += kPrThreads) {
    const int bin = it / nc4, cv = it - bin * nc4;
    PrV4 s{};
    if (roi.ok) {
      const int ph = bin / PW, pw = bin - ph * PW;
      float ws, we, hs, he;
      prroi_bin(roi.sw, roi.bw, pw, ws, we);
      prroi_bin(roi.sh, roi.bh, ph, hs, he);
      const PrGet4 get{f.p + roi.n * f.img + c0 + cv * 4, f.pix, f.row};
      s = prroi_bin_sum<PrV4>(get, f.H, f.W, hs, ws, he, we, nullptr);
      s.x /= roi.area;
      s.y /= roi.area;
      s.z /= roi.area;
      s.w /= roi.area;
    }
    float* st = stage + cv * 4 * bins + bin;
    st[0] = s.x;
    st[bins] = s.y;
    st[2 * bins] = s.z;
    st[3 * bins] = s.w;
  }
  __syncthreads();
  // [nc][bins] of this ROI is one contiguous run of out, 16-byte aligned (C, c0 and nc are multiples of 4)
  float4* o = reinterpret_cast<float4*>(out + ((int64_t)k * f.C + c0) * bins);
  const float4* s4 = reinterpret_cast<const float4*>(stage);
  for (int i = threadIdx.x; i < (nc * bins) >> 2; i += kPrThreads) o[i] = s4[i];
}

__global__ __launch_bounds__(kPrGradThreads) void prroi_grad_roi_kernel(PrFeat f, const float* __restrict__ rois,
                                                                        float scale, int PH, int PW,
                                                                        const float* __restrict__ top,
                                                                        const float* __restrict__ gout,
                                                                        float* __restrict__ grois) {
  __shared__ float red[kPrGradThreads / 64][4];
  const int k = blockIdx.x, bins = PH * PW, c4 = f.C >> 2;
  const PrRoi roi = prroi_roi(rois + (int64_t)k * 5, f.N, scale, PH, PW);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (roi.ok) {   // uniform over the workgroup
    const float* tk = top + (int64_t)k * f.C * bins;
    const float* gk = gout + (int64_t)k * f.C * bins;
    for (int it = threadIdx.x; it < bins * c4; it += kPrGradThreads) {
      const int bin = it / c4, cv = it - bin * c4;
      const int ph = bin / PW, pw = bin - ph * PW;
      const int e = cv * 4 * bins + bin;
      const PrV4 t{tk[e], tk[e + bins], tk[e + 2 * bins], tk[e + 3 * bins]};
      const PrV4 g{gk[e], gk[e + bins], gk[e + 2 * bins], gk[e + 3 * bins]};
      const PrGet4 get{f.p + roi.n * f.img + cv * 4, f.pix, f.row};
      prroi_bin_grad_roi<PrV4>(get, f.H, f.W, roi, ph, pw, PH, PW, scale, t, g, acc);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = acc[j];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = grois + (int64_t)k * 5;
    o[0] = 0.f;
    for (int j = 0; j < 4; ++j) {
      float v = red[0][j];
      for (int w = 1; w < kPrGradThreads / 64; ++w) v += red[w][j];
      o[1 + j] = v;
    }
  }
}

__global__ __launch_bounds__(kPrThreads) void prroi_grad_feat_kernel(int N, int H, int W, int C,
                                                                     const float* __restrict__ rois, int K, float scale,
                                                                     int PH, int PW, const float* __restrict__ gout,
                                                                     float* __restrict__ gfeat) {
  const int c4 = C >> 2, bins = PH * PW;
  const int64_t i = (int64_t)blockIdx.x * kPrThreads + threadIdx.x;
  if (i >= (int64_t)N * H * W * c4) return;
  const int cv = (int)(i % c4), w = (int)((i / c4) % W), h = (int)((i / c4 / W) % H), n = (int)(i / c4 / W / H);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k = 0; k < K; ++k) {
    const PrRoi roi = prroi_roi(rois + (int64_t)k * 5, N, scale, PH, PW);
    if (!roi.ok || roi.n != n) continue;
    const float* gk = gout + ((int64_t)k * C + cv * 4) * bins;
    for (int ph = 0; ph < PH; ++ph) {
      float hs, he;
      prroi_bin(roi.sh, roi.bh, ph, hs, he);
      const float wy = prroi_axis_weight(hs, he, H, h);
      if (wy == 0.f) continue;
      for (int pw = 0; pw < PW; ++pw) {
        float ws, we;
        prroi_bin(roi.sw, roi.bw, pw, ws, we);
        const float wx = prroi_axis_weight(ws, we, W, w);
        if (wx == 0.f) continue;
        const float* g = gk + ph * PW + pw;
        const float cf = wx * wy;
        acc.x += cf * (g[0] / roi.area);
        acc.y += cf * (g[bins] / roi.area);
        acc.z += cf * (g[2 * bins] / roi.area);
        acc.w += cf * (g[3 * bins] / roi.area);
      }
    }
  }
  reinterpret_cast<float4*>(gfeat)[i] = acc;
}

static inline int last_err() { return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP; }
static inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// shape checks shared by the three entries (no HIP call)
static bool bad_shape(int N, int H, int W, int C, int K, float scale, int PH, int PW) {
  return N < 1 || H < 1 || W < 1 || C < 1 || K < 1 || C % 4 || PH < 1 || PH > 8 || PW < 1 || PW > 8 ||
         !prroi_finite(scale) || !(scale > 0.f);
}
static bool bad_pitch(int H, int W, int C, int64_t pix, int64_t row, int64_t img) {
  if (pix < C || pix % 4 || row % 4 || img % 4) return true;
  const int64_t row_extent = (int64_t)(W - 1) * pix + C;
  return row < row_extent || img < (int64_t)(H - 1) * row + row_extent;
}

}  // namespace mmt

using namespace mmt;

extern "C" {

int mmt_prroi_pool_rois(const float* feat, int N, int H, int W, int C, int64_t pix_pitch, int64_t row_pitch,
                        int64_t img_pitch, const float* rois, int K, float spatial_scale, int PH, int PW, float* out,
                        void* stream) {
  if (!feat || !rois || !out || bad_shape(N, H, W, C, K, spatial_scale, PH, PW) ||
      bad_pitch(H, W, C, pix_pitch, row_pitch, img_pitch) || misaligned(feat) || misaligned(out))
    return MMT_E_ARG;
  const int chunk = prroi_chunk(C, PH, PW, K);
  const PrFeat f{feat, pix_pitch, row_pitch, img_pitch, N, H, W, C};
  hipLaunchKernelGGL(prroi_fwd_kernel, dim3(K, (C + chunk - 1) / chunk), dim3(kPrThreads), 0, (hipStream_t)stream, f, rois,
                     spatial_scale, PH, PW, chunk, out);
  return last_err();
}

int mmt_prroi_pool_rois_grad_rois(const float* feat, int N, int H, int W, int C, int64_t pix_pitch, int64_t row_pitch,
                                  int64_t img_pitch, const float* rois, int K, float spatial_scale, int PH, int PW,
                                  const float* out, const float* grad_out, float* grad_rois, void* stream) {
  if (!feat || !rois || !out || !grad_out || !grad_rois || bad_shape(N, H, W, C, K, spatial_scale, PH, PW) ||
      bad_pitch(H, W, C, pix_pitch, row_pitch, img_pitch) || misaligned(feat))
    return MMT_E_ARG;
  const PrFeat f{feat, pix_pitch, row_pitch, img_pitch, N, H, W, C};
  hipLaunchKernelGGL(prroi_grad_roi_kernel, dim3(K), dim3(kPrGradThreads), 0, (hipStream_t)stream, f, rois, spatial_scale, PH,
                     PW, out, grad_out, grad_rois);
  return last_err();
}

int mmt_prroi_pool_rois_grad_feat(int N, int H, int W, int C, const float* rois, int K, float spatial_scale, int PH,
                                  int PW, const float* grad_out, float* grad_feat, void* stream) {
  if (!rois || !grad_out || !grad_feat || bad_shape(N, H, W, C, K, spatial_scale, PH, PW) || misaligned(grad_feat))
    return MMT_E_ARG;
  const int64_t items = (int64_t)N * H * W * (C / 4);
  if (items > (int64_t)0x7fffffff * kPrThreads) return MMT_E_ARG;
  hipLaunchKernelGGL(prroi_grad_feat_kernel, dim3((unsigned)((items + kPrThreads - 1) / kPrThreads)), dim3(kPrThreads), 0,
                     (hipStream_t)stream, N, H, W, C, rois, K, spatial_scale, PH, PW, grad_out, grad_feat);
  return last_err();
}

}  // extern "C"
