// SiamFC per-frame kernels (RGBE/models/siamfc; the published SiamFC tracker, source absent from the
// reference -- parity unpinned beyond the restated algorithm):
//  * siamfc_crop: crop_and_resize for the exemplar / the 3-scale instance pyramid straight from the
//    HBM-resident H x W x C uint8 frame: square window of side round(size) at round(center - (size-1)/2),
//    constant border = the frame's mean colour (cv2.copyMakeBorder BORDER_CONSTANT), cv2 INTER_LINEAR
//    resize, written as float NCHW or NHWC (raw 0..255, what the AlexNet backbone consumes);
//  * siamfc_response: the post-correlation step of TrackerSiamFC.update -- INTER_CUBIC x16 upsampling
//    of every scale's 17x17 response, scale penalty, first-max scale selection, min/sum normalisation,
//    cosine-window blend in double, first-occurrence argmax.
#include "siamfc_dev.h"

namespace mmt {

__global__ __launch_bounds__(256) void siamfc_crop_kernel(const SiamCropArgs a) {
  const int n = blockIdx.y;
  const int O = a.out_sz;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= O * O) return;
  const int oy = idx / O, ox = idx - oy * O;
  const int y0 = a.y0[n], x0 = a.x0[n], S = a.size[n];
  auto px = [&](int r, int x, int c) -> int {
    const int yy = y0 + r, xx = x0 + x;
    if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) return a.pad[c];
    return a.frame[(int64_t)yy * a.stride + (int64_t)xx * a.C + c];
  };
  int u8[3];
  cv_linear_u8(px, S, O, oy, ox, 3, u8);
  if (a.nhwc) {   // [n][O][O][3]: the HIP AlexNet's input layout
    float* o = a.out + ((int64_t)n * O * O + idx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (float)u8[c];
    return;
  }
  float* o = a.out + (int64_t)n * 3 * O * O + idx;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(int64_t)c * O * O] = (float)u8[c];
}

void siamfc_crop(const SiamCropArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(siamfc_crop_kernel, dim3((a.out_sz * a.out_sz + 255) / 256, a.n), dim3(256), 0, s, a);
}

__global__ __launch_bounds__(RT) void siamfc_response_kernel(const SiamRespArgs a) {
  int sid, idx;
  double val;
  siamfc_response_select(a, sid, idx, val);   // siamfc_dev.h: shared with the pooled update (siamfc_pool.hip)
  if (threadIdx.x == 0) {
    a.result[0] = (float)sid;
    a.result[1] = (float)(idx / a.up);
    a.result[2] = (float)(idx % a.up);
    a.result[3] = (float)val;
  }
}

void siamfc_response(const SiamRespArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(siamfc_response_kernel, dim3(1), dim3(RT), 0, s, a);
}

}  // namespace mmt
