// Per-element arithmetic of Precise RoI Pooling (ltr/external/PreciseRoIPooling, restated) shared by the kernels of
// prroi.hip and by host programs (tests/prroi_host_check.cpp): the ROI's validity and bin geometry, the clamped cell
// loops, the closed-form cell integral, the edge interpolation of the box gradient and the per-axis weight of the
// feature gradient.  Plain C++ under a host compiler, __host__ __device__ under hipcc.
//
// Robustness contract (what the three entry points promise for any ROI list):
//  * a ROI is valid when its five values are finite and 0 <= index < N, compared in float before the index is
//    truncated to int; an invalid ROI gives zero outputs and zero gradients;
//  * a ROI whose scaled geometry is not finite (overflow of coordinate * spatial_scale or of the bin area), or with
//    x1 <= x0 or y1 <= y0 (bin area 0), gives zeros as well;
//  * cell loops run over [-1, L - 1] per axis at most: a cell beyond that touches no pixel of the map and adds an
//    exact zero, so no ROI makes a thread read outside the map or visit more than (H + 1)(W + 1) cells per bin.
// The value type V is float (one channel) or PrV4 (four consecutive channels, the layout of a 16-byte load); a
// getter `get(h, w)` returns the V at an in-map pixel and is never called for a pixel outside the map.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MMT_HD __host__ __device__ __forceinline__
#else
#define MMT_HD inline
#endif

namespace mmt {

struct alignas(16) PrV4 {
  float x, y, z, w;
};

MMT_HD void prroi_mad(float& a, float d, float t) { a += d * t; }
MMT_HD void prroi_mad(PrV4& a, const PrV4& d, float t) {
  a.x += d.x * t;
  a.y += d.y * t;
  a.z += d.z * t;
  a.w += d.w * t;
}
MMT_HD void prroi_add(float& a, float b) { a += b; }
MMT_HD void prroi_add(PrV4& a, const PrV4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
MMT_HD int prroi_lanes(const float&) { return 1; }
MMT_HD int prroi_lanes(const PrV4&) { return 4; }
MMT_HD float prroi_comp(const float& v, int) { return v; }
MMT_HD float prroi_comp(const PrV4& v, int j) { return j == 0 ? v.x : (j == 1 ? v.y : (j == 2 ? v.z : v.w)); }

MMT_HD bool prroi_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

// one ROI: scaled start, bin size and bin area; ok == false -> all outputs and gradients of the ROI are zero
struct PrRoi {
  bool ok;
  int n;
  float sw, sh, bw, bh, area;
};

MMT_HD PrRoi prroi_roi(const float* r, int N, float scale, int PH, int PW) {
  PrRoi o{false, 0, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!(prroi_finite(r[0]) && prroi_finite(r[1]) && prroi_finite(r[2]) && prroi_finite(r[3]) && prroi_finite(r[4])))
    return o;
  if (!(r[0] >= 0.f && r[0] < (float)N)) return o;
  o.n = (int)r[0];
  o.sw = r[1] * scale;
  o.sh = r[2] * scale;
  const float ew = r[3] * scale, eh = r[4] * scale;
  o.bw = fmaxf(ew - o.sw, 0.f) / (float)PW;
  o.bh = fmaxf(eh - o.sh, 0.f) / (float)PH;
  o.area = fmaxf(0.f, o.bw * o.bh);
  o.ok = prroi_finite(o.sw) && prroi_finite(o.sh) && prroi_finite(o.bw) && prroi_finite(o.bh) &&
         prroi_finite(o.area) && o.area != 0.f;
  return o;
}

// window [s, e) of bin i along one axis
MMT_HD void prroi_bin(float start, float size, int i, float& s, float& e) {
  s = start + size * (float)i;
  e = s + size;
}

// cells lo <= i < hi a window [s, e) visits on an axis of L samples, clamped to [-1, L - 1] in float before the
// conversion to int (at most L + 1 cells; the cells dropped add exact zeros)
MMT_HD void prroi_cells(float s, float e, int L, int& lo, int& hi) {
  lo = (int)fminf(fmaxf(floorf(s), -1.f), (float)L);
  hi = (int)fminf(fmaxf(ceilf(e), -1.f), (float)L);
}

// integral of the hat of the cell's first (A) / second (B) sample over the window clipped to cell i: both in [0, 1]
MMT_HD float prroi_f(float a, float b) { return a - 0.5f * a * a - b + 0.5f * b * b; }
MMT_HD void prroi_cell_weights(float s, float e, int i, float& A, float& B) {
  const float c0 = fmaxf(s, (float)i), c1 = fminf(e, (float)(i + 1));
  A = prroi_f(c1 - (float)i, c0 - (float)i);
  B = prroi_f((float)(i + 1) - c0, (float)(i + 1) - c1);
}

template <class V, class Get>
MMT_HD V prroi_at(const Get& get, int h, int w, int H, int W) {
  V z{};
  if (h < 0 || w < 0 || h >= H || w >= W) return z;
  return get(h, w);
}

// integral of the bilinear surface over the bin [hs, he) x [ws, we): the sequential sum over cells, w outer, h inner,
// each cell the sum of its four samples in the order (h, w), (h, w + 1), (h + 1, w), (h + 1, w + 1); *cells (may be
// null) receives the number of cells visited
template <class V, class Get>
MMT_HD V prroi_bin_sum(const Get& get, int H, int W, float hs, float ws, float he, float we, int* cells) {
  int wlo, whi, hlo, hhi;
  prroi_cells(ws, we, W, wlo, whi);
  prroi_cells(hs, he, H, hlo, hhi);
  V sum{};
  int n = 0;
  for (int wi = wlo; wi < whi; ++wi) {
    float ax, bx;
    prroi_cell_weights(ws, we, wi, ax, bx);
    if (hlo >= hhi) continue;
    V p0 = prroi_at<V>(get, hlo, wi, H, W), p1 = prroi_at<V>(get, hlo, wi + 1, H, W);
    for (int hi = hlo; hi < hhi; ++hi) {   // a cell's lower samples are the next cell's upper ones: loaded once
      float ay, by;
      prroi_cell_weights(hs, he, hi, ay, by);
      const V q0 = prroi_at<V>(get, hi + 1, wi, H, W), q1 = prroi_at<V>(get, hi + 1, wi + 1, H, W);
      V c{};
      prroi_mad(c, p0, ax * ay);
      prroi_mad(c, p1, bx * ay);
      prroi_mad(c, q0, ax * by);
      prroi_mad(c, q1, bx * by);
      prroi_add(sum, c);
      p0 = q0;
      p1 = q1;
      ++n;
    }
  }
  if (cells) *cells = n;
  return sum;
}

// the bilinear surface on the sample row r at the real abscissa x (0 outside the map's support (-1, W))
template <class V, class Get>
MMT_HD V prroi_edge_row(const Get& get, int r, float x, int H, int W) {
  V v{};
  if (r < 0 || r >= H || !(x > -1.f && x < (float)W)) return v;
  const int f = (int)floorf(x);
  prroi_mad(v, prroi_at<V>(get, r, f, H, W), 1.f - (x - (float)f));
  prroi_mad(v, prroi_at<V>(get, r, f + 1, H, W), 1.f - ((float)(f + 1) - x));
  return v;
}
// ... and on the sample column c at the real ordinate y
template <class V, class Get>
MMT_HD V prroi_edge_col(const Get& get, float y, int c, int H, int W) {
  V v{};
  if (c < 0 || c >= W || !(y > -1.f && y < (float)H)) return v;
  const int f = (int)floorf(y);
  prroi_mad(v, prroi_at<V>(get, f, c, H, W), 1.f - (y - (float)f));
  prroi_mad(v, prroi_at<V>(get, f + 1, c, H, W), 1.f - ((float)(f + 1) - y));
  return v;
}

// integral over [s, t] of the cell (both in [0, 1]) of the line from c1 (at 0) to c2 (at 1), added to acc
template <class V>
MMT_HD void prroi_line_integral(V& acc, float s, float t, const V& c1, const V& c2) {
  prroi_mad(acc, c2, 0.5f * (t * t - s * s));
  prroi_mad(acc, c1, t - 0.5f * t * t - s + 0.5f * s * s);
}

// box gradient of one bin (ph, pw) of a valid ROI: adds to acc[0..3] = d/d(x0, y0, x1, y1) the terms of the V's
// channels in order; top = the pooled output of the bin, g = its incoming gradient
template <class V, class Get>
MMT_HD void prroi_bin_grad_roi(const Get& get, int H, int W, const PrRoi& roi, int ph, int pw, int PH, int PW,
                               float scale, const V& top, const V& g, float acc[4]) {
  float ws, we, hs, he;
  prroi_bin(roi.sw, roi.bw, pw, ws, we);
  prroi_bin(roi.sh, roi.bh, ph, hs, he);
  int wlo, whi, hlo, hhi;
  prroi_cells(ws, we, W, wlo, whi);
  prroi_cells(hs, he, H, hlo, hhi);
  V gx1{}, gx2{}, gy1{}, gy2{};   // the surface integrated along the bin's left, right, top and bottom edges
  for (int hi = hlo; hi < hhi; ++hi) {
    const float s = fmaxf(hs, (float)hi) - (float)hi, t = fminf(he, (float)(hi + 1)) - (float)hi;
    prroi_line_integral(gx1, s, t, prroi_edge_row<V>(get, hi, ws, H, W), prroi_edge_row<V>(get, hi + 1, ws, H, W));
    prroi_line_integral(gx2, s, t, prroi_edge_row<V>(get, hi, we, H, W), prroi_edge_row<V>(get, hi + 1, we, H, W));
  }
  for (int wi = wlo; wi < whi; ++wi) {
    const float s = fmaxf(ws, (float)wi) - (float)wi, t = fminf(we, (float)(wi + 1)) - (float)wi;
    prroi_line_integral(gy1, s, t, prroi_edge_col<V>(get, hs, wi, H, W), prroi_edge_col<V>(get, hs, wi + 1, H, W));
    prroi_line_integral(gy2, s, t, prroi_edge_col<V>(get, he, wi, H, W), prroi_edge_col<V>(get, he, wi + 1, H, W));
  }
  const float dh = he - hs, dw = we - ws;
  const float fx1 = 1.f - (float)pw / (float)PW, fx2 = 1.f - (float)(pw + 1) / (float)PW;
  const float fy1 = 1.f - (float)ph / (float)PH, fy2 = 1.f - (float)(ph + 1) / (float)PH;
  for (int j = 0; j < prroi_lanes(g); ++j) {
    const float gj = prroi_comp(g, j), tj = prroi_comp(top, j);
    if (gj / roi.area == 0.f) continue;
    const float px1 = (-prroi_comp(gx1, j) + dh * tj) / roi.area * scale;
    const float py1 = (-prroi_comp(gy1, j) + dw * tj) / roi.area * scale;
    const float px2 = (prroi_comp(gx2, j) - dh * tj) / roi.area * scale;
    const float py2 = (prroi_comp(gy2, j) - dw * tj) / roi.area * scale;
    acc[0] += (px1 * fx1 + px2 * fx2) * gj;
    acc[1] += (py1 * fy1 + py2 * fy2) * gj;
    acc[2] += (px2 * (1.f - fx2) + px1 * (1.f - fx1)) * gj;
    acc[3] += (py2 * (1.f - fy2) + py1 * (1.f - fy1)) * gj;
  }
}

// feature gradient: the weight of sample p in the window [s, e) of an axis of L samples (the sum of the hat
// integrals of the at most two visited cells that touch p); a bin's coefficient of pixel (h, w) is the product of
// its two axis weights
MMT_HD float prroi_axis_weight(float s, float e, int L, int p) {
  int lo, hi;
  prroi_cells(s, e, L, lo, hi);
  float w = 0.f, A, B;
  if (p >= lo && p < hi) {
    prroi_cell_weights(s, e, p, A, B);
    w += A;
  }
  if (p - 1 >= lo && p - 1 < hi) {
    prroi_cell_weights(s, e, p - 1, A, B);
    w += B;
  }
  return w;
}

}  // namespace mmt
