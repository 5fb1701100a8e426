// Which kernel a GEMM of the tracking path runs on: the tile rules of gemm_plan.cpp as a pure host function
// (no HIP, no environment reads in the decision), so a choice can be printed and tested without a GPU
// (tests/gemm_plan_print.cpp, tests/test_gemm_plan.py).  gemm.hip turns a plan into one launch.
#pragma once
#include <stdint.h>

namespace mmt {

enum Epi : int {
  EPI_BF16 = 0,        // bias -> bf16
  EPI_GELU_BF16 = 1,   // bias, exact GELU -> bf16
  EPI_RESID_F32 = 2,   // C(f32) = R(f32) + (acc + bias)
  EPI_RELU_BF16 = 3,   // bias, ReLU -> bf16            (head conv, BN folded)
  EPI_F32 = 4,         // bias -> f32
  EPI_RELU_F32 = 5,    // bias, ReLU -> f32
  EPI_POS_F32 = 6,     // C(f32) = (acc + bias) + R[m % pos_rows]  (OSTrack patch-embed + pos_embed)
  EPI_PARTIAL = 7,     // internal (split-K): raw fp32 partial sums into the workspace
};
enum AMode : int { A_DENSE = 0, A_CONV3 = 1 };

// Every gemm_kernel configuration the library instantiates: X(BM, BN, WMW, WNW, stages, BK, modes), modes = the
// precisions it is built for (1: bf16, 2: f16x3, 3: both) + 4 where its split-K variant (EPI_PARTIAL) exists too.
// The enumerators, their names and gemm.hip's launch switch are all generated from this list.
#define MMT_GEMM_KERNEL_TILES(X)                                                                                      \
  X(128, 128, 4, 2, 2, 64, 3) X(128, 64, 4, 2, 2, 64, 3) X(128, 64, 2, 2, 2, 64, 3) X(64, 64, 2, 2, 2, 64, 3)         \
  X(64, 32, 4, 1, 2, 64, 3) X(32, 32, 2, 1, 2, 64, 3) X(64, 64, 4, 2, 4, 64, 5) X(64, 64, 4, 2, 3, 64, 6)             \
  X(128, 192, 4, 2, 2, 64, 2) X(128, 128, 4, 2, 2, 32, 2) X(256, 128, 4, 2, 3, 32, 3) X(128, 128, 2, 2, 2, 64, 3)     \
  X(128, 128, 2, 2, 3, 32, 2) X(256, 128, 4, 2, 2, 32, 2) X(128, 256, 2, 4, 3, 32, 2) X(256, 256, 2, 4, 2, 32, 2)     \
  X(128, 128, 4, 2, 3, 32, 3) X(128, 128, 2, 2, 2, 32, 2) X(128, 64, 2, 2, 2, 32, 2) X(128, 128, 4, 2, 4, 32, 3)      \
  X(128, 256, 2, 4, 2, 32, 2) X(64, 64, 2, 2, 8, 32, 2) X(64, 64, 2, 2, 4, 32, 2) X(64, 64, 2, 2, 6, 32, 2)           \
  X(64, 64, 2, 2, 3, 64, 2) X(256, 128, 4, 2, 3, 64, 1) X(256, 128, 4, 2, 2, 64, 1) X(128, 128, 2, 2, 3, 64, 1)       \
  X(256, 256, 4, 2, 2, 64, 1) X(128, 256, 2, 4, 2, 64, 1) X(64, 128, 2, 2, 2, 64, 1) X(128, 64, 2, 2, 4, 32, 1)       \
  X(256, 128, 4, 2, 4, 32, 1) X(128, 64, 4, 2, 3, 64, 1) X(64, 128, 2, 4, 2, 64, 1) X(64, 128, 2, 4, 3, 64, 1)
// The gemm_ring_kernel variants (bf16 only): X(BM, BN, WMW, WNW, ring depth NS, BK, workgroups per CU)
#define MMT_GEMM_RING_TILES(X) \
  X(256, 128, 4, 2, 3, 32, 2) X(128, 128, 4, 2, 4, 32, 2) X(128, 128, 4, 2, 2, 64, 2) X(256, 256, 4, 2, 3, 32, 1) X(256, 128, 4, 2, 2, 64, 1)

#define MMT_TILE_ID(BM, BN, WMW, WNW, ST, BK) T##BM##x##BN##_##WMW##x##WNW##_s##ST##_k##BK
#define MMT_RING_ID(BM, BN, WMW, WNW, NS, BK) RING##BM##x##BN##_##WMW##x##WNW##_s##NS##_k##BK
enum class GemmTile : int {
#define X(BM, BN, WMW, WNW, ST, BK, MODES) MMT_TILE_ID(BM, BN, WMW, WNW, ST, BK),
  MMT_GEMM_KERNEL_TILES(X)
#undef X
#define X(BM, BN, WMW, WNW, NS, BK, WG) MMT_RING_ID(BM, BN, WMW, WNW, NS, BK),
  MMT_GEMM_RING_TILES(X)
#undef X
  PERSIST,    // gemm_persist_kernel, 128 x 128 (bf16, 16-bit epilogues)
  G256,       // gemm256_kernel, 256 x 256 four-phase (bf16)
  G256S,      // gemm256s_kernel<EPI, 4>, 256 x 256 eight-phase (f16x3)
  G256S_320,  // gemm256s_kernel<EPI, 5>, 320 x 256 (f16x3, 16-bit epilogues)
  G128W,      // gemm128w_kernel, 128 x 256 two-group (f16x3, fp32 epilogues)
  NONE,       // no tile: the plan's error says why
};
const char* gemm_tile_name(GemmTile t);

// what tile selection reads of a GEMM
struct GemmShape {
  int M, N, K, groups, amode, epi, split;
  int conc;           // launches of this shape running at once on the chip (0 / 1: alone)
  int has_ws;         // a split-K workspace was given
  int64_t ws_elems;   // its capacity in floats
  int defer_reduce;   // the caller combines split-K slabs itself (EPI_RESID_F32, one group)
};

// the tuning knobs (environment variable MMT_<NAME>, read once per process by gemm_knobs_from_env) and their defaults
struct GemmKnobs {
  int split_cfg = -1;      // MMT_SPLIT_CFG: pin the f16x3 tile (kSplitCfg in gemm_plan.cpp), dense A only
  int t256_min = 128;      // MMT_256S_MIN: fewest 256 x 256 tiles for the eight-phase kernel on the wide GEMMs
  int resid_256s = 1;      // MMT_RESID_256S: residual GEMMs on the eight-phase kernel: 0 never, 1 the rule, 2 always
  int t320 = 1;            // MMT_T320: 320 x 256 tiles: 0 never, 1 the rule, 2 always
  int w256 = 1;            // MMT_W256: 128 x 256 two-group tiles: 0 never, 1 the rule, 2 always
  int persist_min = 1;     // MMT_PERSIST_MIN: persistent kernel from this many tiles per workgroup slot (0: never)
  int split_t128 = 64;     // MMT_SPLIT_T128: f16x3 128-row tiles from this many 128 x 128 tiles
  int t192 = 1;            // MMT_T192: 128 x 192 tiles: 0 never, 1 the rule, 2 always
  int splitk_tiles = 100;  // MMT_SPLITK_TILES: split K below this many 64 x 64 tiles
  int splitk_target = 256; // MMT_SPLITK_TARGET: workgroups aimed at
  int splitk_minkt = 4;    // MMT_SPLITK_MINKT: fewest 64-deep K-tiles per slice
  int splitk_max = 8;      // MMT_SPLITK_MAX: most slices
  int gm = 0;              // MMT_GM: super-tile height of gemm_kernel / gemm128w (0: by K)
  int gm_longk = 4;        // MMT_GM_LONGK: ... for K >= 2048
  int gm256 = 4;           // MMT_GM256: super-tile height of the eight-phase kernel
};
GemmKnobs gemm_knobs_from_env();   // the only getenv of the GEMM code

constexpr int kMaxDeferKs = 8;   // tokens.hip apply_reduce holds at most this many slabs per row
struct GemmPlan {
  GemmTile tile;
  int ksplit;          // K slices (1: none)
  bool defer;          // the slices' slabs stay in the workspace for the consumer: no reduce launch
  int gm;              // tile rows per super-tile of the tile order
  const char* error;   // non-null: nothing to launch (tile == NONE)
};

// force_cfg: mmt_gemm_force_config's pin (-1: the rules)
GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k, int num_cus, int force_cfg);

}  // namespace mmt
