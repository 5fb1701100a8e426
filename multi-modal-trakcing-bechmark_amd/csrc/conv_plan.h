// Which kernel an f16x3 convolution of the DiMP path runs on, with its grid, LDS size and K split: the rules of
// conv_plan.cpp as a pure host function (no HIP, no environment reads in the decision), so a choice can be printed
// and tested without a GPU (tests/conv_plan_print.cpp, tests/test_conv_plan.py).  dimpconv.hip turns a plan into one
// launch (plus the split-K reduce), and takes the kernels' tile constants from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mmt {

constexpr int kMaxGroups = 2, kMaxSplitK = 8;                  // convolutions per launch; K slices
constexpr int kStemTH = 16, kStemTW = 16, kStemMaxKt = 7;      // conv_stem_f16x3_kernel: output tile, K-tiles in LDS
constexpr int kPoolT = 8;                                      // conv_stem_pool_f16x3_kernel: pooled outputs per tile side
constexpr int kPatchMaxPx = 384;                               // conv3x3_patch_f16x3_kernel: patch pixels (48 KB of halves)

enum class ConvKernel : int {
  STEM_POOL,   // conv_stem_pool_f16x3_kernel: the 7 x 7 / stride-2 stem with the max-pool fused (MMT_CONV_POOL)
  PATCH,       // conv3x3_patch_f16x3_kernel<bn>: 3 x 3 / stride 1 / pad 1 from an LDS input patch
  STEM,        // conv_stem_f16x3_kernel: a 4-channel image, 2-D tiles from an LDS input patch
  GENERIC,     // conv_f16x3_kernel<bn, Cin <= 4>: the two-deep gather kernel (any other stem; MMT_CONV_OLD)
  DEEP,        // conv_f16x3_deep_kernel<bn>: the generic conv, and the fused conv3 + downsample
  NONE,        // nothing to launch: the plan's error says why
};
const char* conv_kernel_name(ConvKernel k);

// the switches (environment variables, read once per process by conv_knobs_from_env)
struct ConvKnobs {
  bool nosplit = false;       // MMT_CONV_NOSPLIT: never split K (a batch-invariant summation order)
  bool nopatch = false;       // MMT_CONV_NOPATCH: 3 x 3 convs on the generic kernel (tests: the bitwise comparison)
  bool old_generic = false;   // MMT_CONV_OLD: conv_f16x3_kernel instead of the deep kernel (tests: the bit-exact reference)
};
ConvKnobs conv_knobs_from_env();   // the only getenv of the conv code

struct ConvProblem {
  int N, H, W, Cin, Cout, kh, kw, stride, pad, Kp;   // x [N][H][W][Cin], weights [Cout][Kp]
  int G;                                             // convolutions of this shape in the launch
  bool pool;                                         // MMT_CONV_POOL: the stem writes the max-pooled map
  // a downsample fused into a 1 x 1 conv3: it reads [N][H2][W2][Cin2] at stride2, Kp = Cin + Cin2 (0: none)
  int Cin2, H2, W2, stride2;
  size_t ws_bytes;                                   // split-K workspace given; SIZE_MAX: report what a split would take
};

struct ConvPlan {
  ConvKernel kernel;
  int bn, ks, Ho, Wo;            // output channels per tile, K slices (1: none), output map
  unsigned grid[3];              // 512 threads per workgroup
  size_t lds_bytes;              // dynamic LDS
  int tiles_per_img, patch_px;   // PATCH: tiles per image (0: tiles over the flattened batch), the largest tile's patch
  int tiles_y, tiles_x;          // STEM, STEM_POOL: tiles per image
  int PHo, PWo;                  // STEM_POOL: the pooled map
  bool reduce;                   // conv_splitk_reduce_kernel follows (ks > 1)
  size_t ws_needed;              // bytes of split-K partials this launch writes (0: ks == 1)
  const char* error;             // non-null: nothing to launch (kernel == NONE)
};

int64_t conv_kp(int Cin, int kh, int kw);   // the weights' padded K of a plain conv (a stem tap holds 4 channels)
ConvPlan conv_plan(const ConvProblem& p, const ConvKnobs& k);

}  // namespace mmt
