// SiamFC with the tracker state on the device, n sequences per launch (mmtrack_amd/siamfc.py SiamFCPool).  Per
// frame: siamfc_pool_crop (windows from the per-slot state, each sequence's own frame) -> the AlexNet backbone ->
// xcorr_nhwc_group (a sequence's scales share its exemplar) -> siamfc_pool_update (the selection of
// siamfc_response_kernel, then the state law of TrackerSiamFC.update and the result record).  The crop, the
// correlation sum and the selection are the sequential kernels' own device code (cvresize.h, siamfc_dev.h), so a
// pool of any size gives the sequential tracker's bits.
#include "siamfc_dev.h"

namespace mmt {

constexpr double kMaxSide = 1048576.0;   // 2^20: a larger (or non-finite, or < 1) side is a degenerate window

// The window of `st` at scale factor f, as TrackerSiamFC._crop forms it: side = round(x_sz * f) (half to even),
// corner = np.round(center - (side - 1) / 2).  false: degenerate (y0 = x0 = side = 0).  A corner outside
// +-2^30 (a centre that ran away or is not a number) is clamped there: such a window lies wholly outside any frame
// and corner + side stays inside int.
__device__ __forceinline__ bool siam_window(const SiamState& st, double f, int& y0, int& x0, int& side) {
#pragma clang fp contract(off)
  const double s = rint(st.x_sz * f);
  if (!(s >= 1.0) || !(s <= kMaxSide)) {   // NaN fails both
    y0 = x0 = side = 0;
    return false;
  }
  const double half = (s - 1.0) / 2.0, lim = 1073741824.0;
  const double cy = rint(st.center[0] - half), cx = rint(st.center[1] - half);
  y0 = cy >= -lim && cy <= lim ? (int)cy : (int)lim;
  x0 = cx >= -lim && cx <= lim ? (int)cx : (int)lim;
  side = (int)s;
  return true;
}

// any window of the sequence degenerate: the sequence is not advanced this frame.  The flag is this function of the
// slot's state in device memory: the crop and the update of a frame read the same state, so they agree.
__device__ __forceinline__ bool siam_degenerate(const SiamState& st, const SiamParams& p) {
  int y0, x0, side;
  bool bad = false;
  for (int s = 0; s < p.scale_num; ++s) bad |= !siam_window(st, p.scale_factors[s], y0, x0, side);
  return bad;
}

__global__ __launch_bounds__(256) void siamfc_pool_crop_kernel(const SiamState* __restrict__ states,
                                                               const SiamFrame* __restrict__ frames,
                                                               const SiamParams p, float* __restrict__ out,
                                                               int* __restrict__ windows) {
  const int e = blockIdx.y, q = e / p.scale_num, sc = e - q * p.scale_num;
  const int O = p.instance_sz;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const SiamState st = states[q];
  int y0, x0, S;
  const bool ok = siam_window(st, p.scale_factors[sc], y0, x0, S);
  if (windows && idx == 0) {
    int* w = windows + (int64_t)e * 3;
    w[0] = y0;
    w[1] = x0;
    w[2] = S;
  }
  if (idx >= O * O) return;
  float* o = out + ((int64_t)e * O * O + idx) * 3;
  if (!ok) {
    o[0] = o[1] = o[2] = 0.f;
    return;
  }
  const SiamFrame f = frames[q];
  // a descriptor the kernel cannot index reads as border everywhere
  const bool usable = f.data && f.H > 0 && f.W > 0 && f.C >= 3 && f.stride >= (int64_t)f.W * f.C;
  const int H = usable ? f.H : 0, W = usable ? f.W : 0;
  int pad[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) pad[c] = min(max(st.pad[c], 0), 255);
  const int oy = idx / O, ox = idx - oy * O;
  auto px = [&](int r, int x, int c) -> int {
    const int yy = y0 + r, xx = x0 + x;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) return pad[c];
    return f.data[(int64_t)yy * f.stride + (int64_t)xx * f.C + c];
  };
  int u8[3];
  cv_linear_u8(px, S, O, oy, ox, 3, u8);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (float)u8[c];
}

// xcorr_nhwc_kernel's layout (a workgroup: one entry, 4 output pixels, one wave each, the exemplar in the LDS) with
// entry b reading the exemplar of its sequence b / group.  Letting a workgroup fill the LDS once for all of a
// sequence's scales, or for more pixels, was measured slower at every batch size (the 36 KB
// fill comes from L2 and is cheap, the outputs a wave then computes one after the other are not), so the layout
// stays.  xcorr_nhwc_pixel's lane sums and butterfly: xcorr_nhwc_kernel's bits.
__global__ __launch_bounds__(256) void xcorr_nhwc_group_kernel(const float* __restrict__ Z, int64_t z_bstride, int group,
                                                               const float* __restrict__ X, float* __restrict__ out,
                                                               int C, int hz, int wz, int hx, int wx, float scale,
                                                               float bias) {
  extern __shared__ __attribute__((aligned(16))) float zsh[];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int ho = hx - hz + 1, wo = wx - wz + 1;
  const int n = hz * wz * C;
  const float* zb = Z + (b / group) * z_bstride;
  for (int i = threadIdx.x; i < n; i += 256) zsh[i] = zb[i];
  __syncthreads();
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= ho * wo) return;
  const int y = p / wo, x = p - y * wo;
  const float* xb = X + (int64_t)b * hx * wx * C;
  const float acc = xcorr_nhwc_pixel(xb, zsh, C, hz, wz, wx, y, x, lane);
  if (lane == 0) out[(int64_t)b * ho * wo + p] = acc * scale + bias;
}

__global__ __launch_bounds__(RT) void siamfc_pool_update_kernel(const float* __restrict__ resp, const SiamParams p,
                                                                float penalty, float one_minus_wi,
                                                                const double* __restrict__ hann1d,
                                                                float* __restrict__ scratch, SiamState* states,
                                                                SiamResult* results, SiamResult* host_results) {
#pragma clang fp contract(off)   // the state law in numpy's separate float64 roundings
  const int q = blockIdx.x, up = p.response_up * p.response_sz;
  __shared__ int degenerate;
  if (threadIdx.x == 0) degenerate = siam_degenerate(states[q], p) ? 1 : 0;
  __syncthreads();
  const bool bad = degenerate != 0;   // uniform over the workgroup
  int sid = 0, idx = 0;
  double val = 0.0;
  if (!bad) {
    SiamRespArgs a;
    a.resp = resp + (int64_t)q * p.scale_num * p.response_sz * p.response_sz;
    a.n = p.scale_num;
    a.r = p.response_sz;
    a.up = up;
    a.penalty = penalty;
    a.one_minus_wi = one_minus_wi;
    a.wi = p.window_influence;
    a.hann_sum = p.hann_sum;
    a.hann1d = hann1d;
    a.scratch = scratch + (int64_t)q * p.scale_num * up * up;
    a.result = nullptr;
    siamfc_response_select(a, sid, idx, val);
  }
  if (threadIdx.x != 0) return;
  SiamState st = states[q];
  SiamResult r{};
  if (bad) {
    r.err = 1;
  } else {
    const int row = idx / up, col = idx % up;
    const double f = p.scale_factors[sid];
    double d[2] = {(double)row - (double)(up - 1) / 2.0, (double)col - (double)(up - 1) / 2.0};
    for (int k = 0; k < 2; ++k) {
      d[k] = d[k] * (double)p.total_stride / (double)p.response_up;
      d[k] = d[k] * st.x_sz * f / (double)p.instance_sz;
      st.center[k] = st.center[k] + d[k];
    }
    const double scale = (1.0 - p.scale_lr) * 1.0 + p.scale_lr * f;
    st.target_sz[0] = st.target_sz[0] * scale;
    st.target_sz[1] = st.target_sz[1] * scale;
    st.z_sz = st.z_sz * scale;
    st.x_sz = st.x_sz * scale;
    st.frame_num += 1;
    states[q] = st;
    r.value = (float)val;
    r.scale_id = sid;
    r.row = row;
    r.col = col;
  }
  r.box[0] = st.center[1] + 1.0 - (st.target_sz[1] - 1.0) / 2.0;
  r.box[1] = st.center[0] + 1.0 - (st.target_sz[0] - 1.0) / 2.0;
  r.box[2] = st.target_sz[1];
  r.box[3] = st.target_sz[0];
  results[q] = r;
  if (host_results) {
    host_results[q] = r;
    __threadfence_system();   // the host reads the record after the stream's event
  }
}

void siamfc_pool_crop(const SiamState* states, const SiamFrame* frames, int n, const SiamParams& p, float* out,
                      int* windows, hipStream_t s) {
  const int O = p.instance_sz;
  hipLaunchKernelGGL(siamfc_pool_crop_kernel, dim3((O * O + 255) / 256, n * p.scale_num), dim3(256), 0, s, states,
                     frames, p, out, windows);
}

void xcorr_nhwc_group(const float* Z, int64_t z_bstride, int group, const float* X, float* out, int B, int C, int hz,
                      int wz, int hx, int wx, float scale, float bias, hipStream_t s) {
  const int n = (hx - hz + 1) * (wx - wz + 1);
  hipLaunchKernelGGL(xcorr_nhwc_group_kernel, dim3((n + 3) / 4, B), dim3(256), (size_t)hz * wz * C * sizeof(float), s, Z,
                     z_bstride, group, X, out, C, hz, wz, hx, wx, scale, bias);
}

void siamfc_pool_update(const float* resp, int n, const SiamParams& p, const double* hann1d, float* scratch,
                        SiamState* states, SiamResult* results, SiamResult* host_results, hipStream_t s) {
  hipLaunchKernelGGL(siamfc_pool_update_kernel, dim3(n), dim3(RT), 0, s, resp, p, p.scale_penalty,
                     (float)(1.0 - p.window_influence), hann1d, scratch, states, results, host_results);
}

}  // namespace mmt
