// csrc/iounet_dev.h on the host: the box kernels' own arithmetic (xywh -> ROI, the fold of the two levels' ROI
// gradients into the box gradient, one ascent step) and the K split, built with -fsanitize=address,undefined by
// tests/test_iounet_host.py.
//   iounet_host_check P step_pos step_size < lines     one "x y w h  g3_x0 g3_y0 g3_x1 g3_y1  g4_x0 g4_y0 g4_x1 g4_y1"
//                                                      per box (strtof: nan, inf, -inf, 1e30)
// prints per box "roi" (5 values), "grad" (4) and "step" (4) with %.9g, then "ksplit" of the Kd values 4 .. 6400.
// Every buffer is a heap block of the exact size, so an index past a box's values is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "iounet_dev.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int P = atoi(argv[1]);
  const float step_pos = strtof(argv[2], nullptr), step_size = strtof(argv[3], nullptr);
  if (P < 1) return 2;
  std::vector<float> vals;
  char tok[64];
  while (scanf("%63s", tok) == 1) vals.push_back(strtof(tok, nullptr));
  if (vals.size() % 12) return 2;
  const int R = (int)(vals.size() / 12);
  for (int r = 0; r < R; ++r) {
    float* box = new float[4];
    float* g3 = new float[5];
    float* g4 = new float[5];
    float* roi = new float[5];
    float* gb = new float[4];
    float* out = new float[4];
    g3[0] = g4[0] = 0.f;
    for (int j = 0; j < 4; ++j) {
      box[j] = vals[12 * r + j];
      g3[1 + j] = vals[12 * r + 4 + j];
      g4[1 + j] = vals[12 * r + 8 + j];
    }
    mmt::iou_box_to_roi(box, r / P, roi);
    mmt::iou_fold_grad(g3, g4, gb);
    mmt::iou_step(box, gb, step_pos, step_size, out);
    printf("roi %.9g %.9g %.9g %.9g %.9g\n", roi[0], roi[1], roi[2], roi[3], roi[4]);
    printf("grad %.9g %.9g %.9g %.9g\n", gb[0], gb[1], gb[2], gb[3]);
    printf("step %.9g %.9g %.9g %.9g\n", out[0], out[1], out[2], out[3]);
    delete[] box;
    delete[] g3;
    delete[] g4;
    delete[] roi;
    delete[] gb;
    delete[] out;
  }
  printf("ksplit %d %d %d %d %d %d\n", mmt::iou_ksplit(4), mmt::iou_ksplit(128), mmt::iou_ksplit(132), mmt::iou_ksplit(360),
         mmt::iou_ksplit(2304), mmt::iou_ksplit(6400));
  return 0;
}
