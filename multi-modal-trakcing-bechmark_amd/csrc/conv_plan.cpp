// The launch rules of the f16x3 convolutions, top to bottom in the order they apply.
#include "conv_plan.h"

#include <stdlib.h>

#include <algorithm>

namespace mmt {

const char* conv_kernel_name(ConvKernel k) {
  static const char* const names[] = {"stem_pool", "patch", "stem", "generic", "deep", "none"};
  return names[(int)k];
}

ConvKnobs conv_knobs_from_env() {
  ConvKnobs k;
  k.nosplit = getenv("MMT_CONV_NOSPLIT") != nullptr;
  k.nopatch = getenv("MMT_CONV_NOPATCH") != nullptr;
  k.old_generic = getenv("MMT_CONV_OLD") != nullptr;
  return k;
}

int64_t conv_kp(int Cin, int kh, int kw) {
  const bool stem = Cin == 3 || Cin == 4;   // 4: a 3-channel image padded with a zero channel
  return ((int64_t)kh * kw * (stem ? 4 : Cin) + 31) / 32 * 32;
}

namespace {

const char* conv_shape(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int& Ho, int& Wo) {
  const bool stem = Cin == 3 || Cin == 4;
  if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cout % 64 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 ||
      (!stem && Cin % 32))
    return "sizes must be positive, Cout a multiple of 64, Cin 3, 4 or a multiple of 32";
  const int64_t K = (int64_t)kh * kw * (stem ? 4 : Cin);
  Ho = (H + 2 * pad - kh) / stride + 1;
  Wo = (W + 2 * pad - kw) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return "the kernel does not fit the padded input";
  const int64_t M = (int64_t)N * Ho * Wo;
  if (M > (int64_t)1 << 30 || (int64_t)Cout * K > (int64_t)1 << 30) return "more than 2^30 output pixels or weights";
  return nullptr;
}

// output channels per tile: 128 everywhere but the stem
int conv_bn(int Cin, int Cout) { return Cin <= 4 || Cout % 128 ? 64 : 128; }

// the 3 x 3 / stride-1 patch kernel's geometry: *tiles = the launch's tiles, *tiles_per_img = tiles per image (128
// raster pixels each) or 0 for tiles over the flattened batch (chosen when the images' partial last tiles would waste
// more than 4 % of the rows and every batch tile's patch fits -- HW >= 128, so a tile spans at most two images);
// returns the largest tile's patch (pixels), 0 when the shape is not one it runs
int patch_plan(int N, int H, int W, int Cin, int kh, int kw, int stride, int pad, int* tiles, int* tiles_per_img) {
  if (kh != 3 || kw != 3 || stride != 1 || pad != 1 || Cin % 32 || Cin < 32) return 0;
  const int HW = H * W, tpi = (HW + 127) / 128, PW = W + 2;
  int px = 0;
  for (int tl = 0; tl < tpi; ++tl) {
    const int o0 = tl * 128, o1 = std::min(o0 + 128, HW);
    px = std::max(px, ((o1 - 1) / W - o0 / W + 3) * PW);
  }
  const int64_t total = (int64_t)N * HW, gtiles = (total + 127) / 128;
  if (HW >= 128 && (int64_t)N * tpi * 128 > total * 104 / 100 && N > 1) {
    int gpx = 0;
    for (int64_t tl = 0; tl < gtiles; ++tl) {
      const int64_t g0 = tl * 128, gend = std::min(g0 + 128, total);
      const int64_t nA = g0 / HW, y0 = (g0 - nA * HW) / W;
      const int64_t aend = std::min(gend, (nA + 1) * HW) - nA * HW;
      int rows = (int)((aend - 1) / W - y0 + 3);
      if (gend > (nA + 1) * HW) rows += (int)((gend - (nA + 1) * HW - 1) / W + 3);
      gpx = std::max(gpx, rows * PW);
    }
    if (gpx <= kPatchMaxPx) {
      *tiles = (int)gtiles;
      *tiles_per_img = 0;
      return gpx;
    }
  }
  if (px > kPatchMaxPx) return 0;
  *tiles = N * tpi;
  *tiles_per_img = tpi;
  return px;
}

// K slices for a launch of `tiles` output tiles over nk K-tiles, when the tiles alone leave the GPU's 256 CUs
// under-filled: the split whose last round of workgroups (over kSlots slots) is fullest (ties: the fewest
// slices), at least 8 K-tiles per slice.  256 slots (one workgroup per CU) measured +1 % over 512 and level
// with no split at all once the two backbones share a launch (profiles/r03_ab_conv_slots.txt)
int conv_pick_ks(int64_t tiles, int nk, bool nosplit) {
  // slots: 256 (one workgroup per CU): a launch with a workgroup for every CU is not split.  (Round 3 counted the
  // long-K layers -- >= 72 K-tiles: layer3's 3 x 3 convs and the clf conv -- two per CU, splitting them 4 ways at 32
  // images; with the patch kernel's tiles over the flattened batch, 324 tiles, no split measured +0.3 % on the mfDiMP
  // line and drops the 7 slice-reduce launches of a step, tools/runs_r4/r4_run19.sh.  Small batches still split.)
  // The clf conv's K (288 K-tiles) is long enough that two slices per CU still pay: 512 slots from 144 K-tiles
  // (unsplit 324 us against 254 + 14 us, r4_run20).
  const int64_t kSlots = nk >= 144 ? 512 : 256;
  if (tiles >= kSlots || nosplit) return 1;
  int best = 1;
  double best_eff = 0.0;
  for (int ks = 1; ks <= kMaxSplitK && nk / ks >= 8; ++ks) {
    const int64_t w = tiles * ks, rounds = (w + kSlots - 1) / kSlots;
    const double eff = (double)w / (double)(rounds * kSlots);
    if (eff > best_eff + 0.02) {
      best_eff = eff;
      best = ks;
    }
  }
  return best;
}

ConvPlan reject(const char* why) { return ConvPlan{ConvKernel::NONE, 0, 1, 0, 0, {0, 0, 0}, 0, 0, 0, 0, 0, 0, 0, false, 0, why}; }

}  // namespace

ConvPlan conv_plan(const ConvProblem& p, const ConvKnobs& k) {
  if (p.G < 1 || p.G > kMaxGroups) return reject("1 or 2 convolutions per launch");
  const bool ds = p.Cin2 > 0 || p.H2 || p.W2 || p.stride2;
  // conv3 is 1 x 1 / stride 1 over [N][H][W][Cin]; the downsample 1 x 1 / stride2 over [N][H2][W2][Cin2] lands on
  // the same H x W grid; the weights hold both K ranges
  if (ds && (p.pool || p.kh != 1 || p.kw != 1 || p.stride != 1 || p.pad != 0 || p.Cin < 32 || p.Cin % 32 || p.Cin2 < 32 ||
             p.Cin2 % 32 || p.stride2 < 1 || p.H2 <= 0 || p.W2 <= 0 || (p.H2 - 1) / p.stride2 + 1 != p.H ||
             (p.W2 - 1) / p.stride2 + 1 != p.W || p.Kp != p.Cin + p.Cin2))
    return reject("fused downsample: 1 x 1 convs over channel multiples of 32, x2 strided onto the same grid, Kp = Cin + Cin2");
  const int cin = ds ? p.Kp : p.Cin;   // channels of the launch's one tap
  ConvPlan r = reject(nullptr);
  if (const char* why = conv_shape(p.N, p.H, p.W, cin, p.Cout, p.kh, p.kw, p.stride, p.pad, r.Ho, r.Wo)) return reject(why);
  if (p.Kp != conv_kp(cin, p.kh, p.kw)) return reject("Kp is not the shape's K padded to 32");
  if (ds && (int64_t)p.N * p.H2 * p.W2 * p.Cin2 > ((int64_t)1 << 29)) return reject("x2 past 32-bit buffer offsets");
  const int G = p.G, Ho = r.Ho, Wo = r.Wo;
  const int64_t M = (int64_t)p.N * Ho * Wo;
  if (p.pool) {
    // the 7 x 7 / stride-2 stem with the 3 x 3 / stride-2 / pad-1 max-pool fused; y is the pooled map
    if (p.Cin != 4 || p.Cout != 64 || p.kh != 7 || p.kw != 7 || p.stride != 2 || p.Kp != 224)
      return reject("the pooled stem is 7 x 7 / stride 2 over 4 channels to 64");
    r.kernel = ConvKernel::STEM_POOL;
    r.bn = 64;
    r.PHo = (Ho - 1) / 2 + 1, r.PWo = (Wo - 1) / 2 + 1;
    r.tiles_y = (r.PHo + kPoolT - 1) / kPoolT, r.tiles_x = (r.PWo + kPoolT - 1) / kPoolT;
    r.grid[0] = (unsigned)(p.N * r.tiles_y * r.tiles_x), r.grid[1] = 1, r.grid[2] = (unsigned)G;
    return r;
  }
  const int bn = r.bn = conv_bn(cin, p.Cout), gn = p.Cout / bn, nk = p.Kp / 32;
  int ptiles = 0;
  r.patch_px = k.nopatch ? 0 : patch_plan(p.N, p.H, p.W, cin, p.kh, p.kw, p.stride, p.pad, &ptiles, &r.tiles_per_img);
  // M tiles of the launch (the patch kernel has its own tiling; its slices are ranges of 32-channel chunks) and its K split
  const int64_t gm = (M + 127) / 128;
  int ks = r.patch_px ? std::min(conv_pick_ks((int64_t)ptiles * gn * G, nk, k.nosplit), cin / 32)
                      : conv_pick_ks(gm * gn * G, nk, k.nosplit);
  if (ks > 1 && p.ws_bytes < (size_t)(ks * G * M * (int64_t)p.Cout * 4)) ks = 1;   // workspace too small: no split
  r.ks = ks;
  r.reduce = ks > 1;
  r.ws_needed = ks > 1 ? (size_t)(ks * G * M * (int64_t)p.Cout * 4) : 0;
  r.grid[0] = (unsigned)gm, r.grid[1] = (unsigned)gn, r.grid[2] = (unsigned)(G * ks);
  if (r.patch_px) {
    r.kernel = ConvKernel::PATCH;
    r.grid[0] = (unsigned)ptiles;
    r.lds_bytes = (size_t)(2 * kPatchMaxPx * 32 + 2 * 2 * bn * 32) * 2;   // 80 KB (bn 128): two per CU
  } else if (p.Cin == 4 && p.Cout == 64 && ks == 1 && p.kh <= 7 && p.kw <= 7 && p.stride <= 2 && nk <= kStemMaxKt) {
    r.kernel = ConvKernel::STEM;
    r.tiles_y = (Ho + kStemTH - 1) / kStemTH, r.tiles_x = (Wo + kStemTW - 1) / kStemTW;
    r.grid[0] = (unsigned)(r.tiles_y * r.tiles_x * p.N), r.grid[1] = 1, r.grid[2] = (unsigned)G;
  } else if (p.Cin <= 4 || (k.old_generic && !ds)) {   // (only the deep kernel reads a second source)
    r.kernel = ConvKernel::GENERIC;
  } else {
    r.kernel = ConvKernel::DEEP;   // M x N tiles flattened (the kernel's XCD-aware tile order)
    r.grid[0] = (unsigned)(gm * gn), r.grid[1] = 1;
  }
  return r;
}

}  // namespace mmt
