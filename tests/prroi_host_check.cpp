// Host evaluation of csrc/prroi_dev.h, the arithmetic the PrRoIPool kernels run (tests/test_prroi_host.py builds this
// with -fsanitize=address,undefined and feeds it an adversarial ROI list).
//   prroi_host_check N H W C PH PW scale < rois      one "index x0 y0 x1 y1" per line (strtof: nan, inf, -inf, 1e30)
// The map is feat[n][h][w][c] = ((131 n + 31 h + 17 w + 7 c) % 23 - 11) / 8 in an exact-size heap block, so the
// sanitizer's redzones are its guard bytes, and the getter aborts on a pixel outside the map; grad_out[k][c][ph][pw] =
// ((29 k + 13 c + 5 ph + 3 pw) % 17 - 8) / 4.  Prints per ROI "out" (C PH PW values), "grad" (5 values), and at the end
// "max_cells", the largest number of cells any bin visited.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prroi_dev.h"

using namespace mmt;

struct Get {
  const float* base;   // image n, channel c
  int H, W, C;
  float operator()(int h, int w) const {
    if (h < 0 || w < 0 || h >= H || w >= W) {
      std::fprintf(stderr, "read outside the map: (%d, %d)\n", h, w);
      std::abort();
    }
    return base[((int64_t)h * W + w) * C];
  }
};

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const int N = std::atoi(argv[1]), H = std::atoi(argv[2]), W = std::atoi(argv[3]), C = std::atoi(argv[4]);
  const int PH = std::atoi(argv[5]), PW = std::atoi(argv[6]);
  const float scale = std::strtof(argv[7], nullptr);
  float* feat = static_cast<float*>(std::malloc(sizeof(float) * N * H * W * C));
  for (int n = 0; n < N; ++n)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w)
        for (int c = 0; c < C; ++c)
          feat[(((int64_t)n * H + h) * W + w) * C + c] = (float)((131 * n + 31 * h + 17 * w + 7 * c) % 23 - 11) / 8.f;
  int max_cells = 0, k = 0;
  char tok[5][64];
  while (std::scanf("%63s %63s %63s %63s %63s", tok[0], tok[1], tok[2], tok[3], tok[4]) == 5) {
    float r[5];
    for (int i = 0; i < 5; ++i) r[i] = std::strtof(tok[i], nullptr);
    const PrRoi roi = prroi_roi(r, N, scale, PH, PW);
    std::vector<float> out((size_t)C * PH * PW, 0.f);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (roi.ok) {
      for (int c = 0; c < C; ++c)
        for (int ph = 0; ph < PH; ++ph)
          for (int pw = 0; pw < PW; ++pw) {
            float ws, we, hs, he;
            prroi_bin(roi.sw, roi.bw, pw, ws, we);
            prroi_bin(roi.sh, roi.bh, ph, hs, he);
            const Get get{feat + (int64_t)roi.n * H * W * C + c, H, W, C};
            int cells = 0;
            const float v = prroi_bin_sum<float>(get, H, W, hs, ws, he, we, &cells) / roi.area;
            if (cells > max_cells) max_cells = cells;
            out[((size_t)c * PH + ph) * PW + pw] = v;
            const float g = (float)((29 * k + 13 * c + 5 * ph + 3 * pw) % 17 - 8) / 4.f;
            prroi_bin_grad_roi<float>(get, H, W, roi, ph, pw, PH, PW, scale, v, g, acc);
            // the feature gradient's axis weights over every sample of both axes
            for (int w = 0; w < W; ++w) (void)prroi_axis_weight(ws, we, W, w);
            for (int h = 0; h < H; ++h) (void)prroi_axis_weight(hs, he, H, h);
          }
    }
    std::printf("out");
    for (float v : out) std::printf(" %.9g", v);
    std::printf("\ngrad 0 %.9g %.9g %.9g %.9g\n", acc[0], acc[1], acc[2], acc[3]);
    ++k;
  }
  std::printf("max_cells %d\n", max_cells);
  std::free(feat);
  return 0;
}
