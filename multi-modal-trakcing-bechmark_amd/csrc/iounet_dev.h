// Per-box arithmetic of the IoU-Net box ascent (ltr/models/bbreg/atom_iou_net.py:118-124 and
// pytracking/tracker/dimp/dimp.py:727-752, restated) shared by the box kernels of iounet.hip and by host programs
// (tests/iounet_host_check.cpp), and the K split of the row-linear kernel, which the host-side workspace sizes and
// the launches both read.  Plain C++ under a host compiler, __host__ __device__ under hipcc.
//
// Every sum and product below is one rounded float32 operation in the written order (no contraction into an fma),
// which is what the reference's sequence of torch operations computes: the fused ascent then gives the bits of the
// same loop written over predict_iou.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IOU_HD __host__ __device__ __forceinline__
#else
#define IOU_HD inline
#endif

namespace mmt {

// one rounded float32 sum / product, never contracted into an fma with its neighbours: clang (hipcc's host and
// device passes) honours the pragma; another host compiler gets a volatile temporary
IOU_HD float iou_add(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return a + b;
#else
  volatile float s = a + b;
  return s;
#endif
}
IOU_HD float iou_mul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
  return a * b;
#else
  volatile float p = a * b;
  return p;
#endif
}

// box (x, y, w, h) of sequence `seq` -> ROI (batch index, x0, y0, x1, y1); any value passes through (a NaN, an
// infinite or a negative size makes a ROI that PrRoIPool pools to zeros)
IOU_HD void iou_box_to_roi(const float* box, int seq, float* roi) {
  roi[0] = (float)seq;
  roi[1] = box[0];
  roi[2] = box[1];
  roi[3] = iou_add(box[0], box[2]);
  roi[4] = iou_add(box[1], box[3]);
}

// the ROI gradients (0, g_x0, g_y0, g_x1, g_y1) of the two pooling levels -> the gradient to (x, y, w, h):
// x0 = x and x1 = x + w, so d/dx = g_x0 + g_x1 and d/dw = g_x1; the two levels are summed last
IOU_HD void iou_fold_grad(const float* g3, const float* g4, float* gbox) {
  gbox[0] = iou_add(iou_add(g3[1], g3[3]), iou_add(g4[1], g4[3]));
  gbox[1] = iou_add(iou_add(g3[2], g3[4]), iou_add(g4[2], g4[4]));
  gbox[2] = iou_add(g3[3], g4[3]);
  gbox[3] = iou_add(g3[4], g4[4]);
}

// box + step * grad * (w, h, w, h) with the pre-update w, h; step_pos scales x, y and step_size w, h
IOU_HD void iou_step(const float* box, const float* gbox, float step_pos, float step_size, float* out) {
  const float w = box[2], h = box[3];
  out[0] = iou_add(box[0], iou_mul(iou_mul(step_pos, gbox[0]), w));
  out[1] = iou_add(box[1], iou_mul(iou_mul(step_pos, gbox[1]), h));
  out[2] = iou_add(box[2], iou_mul(iou_mul(step_size, gbox[2]), w));
  out[3] = iou_add(box[3], iou_mul(iou_mul(step_size, gbox[3]), h));
}

// The row-linear kernel's K split: a workgroup sums one slice of kIouSlice columns of Kd (four waves, a quarter
// each), so the number of slices -- and with it every partial sum's content and the order they are added in --
// depends on the weight shape only, never on the number of rows.
constexpr int kIouSlice = 128;
IOU_HD int iou_ksplit(int Kd) { return (Kd + kIouSlice - 1) / kIouSlice; }

}  // namespace mmt
