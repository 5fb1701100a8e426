// The tile rules of the tracking path's GEMMs, top to bottom in the order they apply.
#include "gemm_plan.h"

#include <stdlib.h>

namespace mmt {

namespace {

struct TileInfo { const char* name; int bm, bn, bk, depth, modes; };   // depth: LDS stages / ring depth
const TileInfo kTiles[] = {
#define X(BM, BN, WMW, WNW, ST, BK, MODES) {#BM "x" #BN "_" #WMW "x" #WNW "_s" #ST "_k" #BK, BM, BN, BK, ST, MODES},
    MMT_GEMM_KERNEL_TILES(X)
#undef X
#define X(BM, BN, WMW, WNW, NS, BK, WG) {"ring" #BM "x" #BN "_" #WMW "x" #WNW "_s" #NS "_k" #BK, BM, BN, BK, NS, 1},
    MMT_GEMM_RING_TILES(X)
#undef X
    {"persist", 128, 128, 64, 2, 1}, {"gemm256", 256, 256, 64, 2, 1}, {"gemm256s", 256, 256, 32, 2, 2},
    {"gemm256s_320", 320, 256, 32, 2, 2}, {"gemm128w", 128, 256, 32, 3, 2}, {"none", 1, 1, 1, 0, 0}};
const TileInfo& info(GemmTile t) { return kTiles[(int)t]; }

#define T(BM, BN, WMW, WNW, ST, BK) GemmTile::MMT_TILE_ID(BM, BN, WMW, WNW, ST, BK)
#define RING(BM, BN, WMW, WNW, NS, BK) GemmTile::MMT_RING_ID(BM, BN, WMW, WNW, NS, BK)
// MMT_SPLIT_CFG number -> f16x3 tile (tuning: tools/sweep_split_cfg_*.sh, tools/bench_f16x3.py); 15: only N >= 2048
const GemmTile kSplitCfg[20] = {
    T(128, 128, 4, 2, 2, 64), T(256, 128, 4, 2, 3, 32), T(128, 128, 2, 2, 2, 64), T(128, 128, 2, 2, 3, 32),
    T(256, 128, 4, 2, 2, 32), T(128, 256, 2, 4, 3, 32), T(256, 256, 2, 4, 2, 32), T(128, 128, 4, 2, 3, 32),
    T(128, 64, 2, 2, 2, 64),  T(128, 128, 4, 2, 2, 32), T(128, 128, 2, 2, 2, 32), T(128, 64, 2, 2, 2, 32),
    T(128, 128, 4, 2, 4, 32), T(128, 256, 2, 4, 2, 32), GemmTile::G256S,          GemmTile::G256S,
    T(64, 64, 2, 2, 8, 32),   T(64, 64, 2, 2, 4, 32),   T(64, 64, 2, 2, 6, 32),   T(64, 64, 2, 2, 3, 64)};
// mmt_gemm_force_config number -> bf16 tile (0: none); 128 / 256 / 320 pin f16x3 tiles (gemm_plan below)
const GemmTile kForceCfg[25] = {
    GemmTile::NONE,           T(256, 128, 4, 2, 3, 64), T(256, 128, 4, 2, 2, 64), T(128, 128, 2, 2, 2, 64),
    T(128, 128, 2, 2, 3, 64), T(128, 128, 4, 2, 2, 64), T(256, 256, 4, 2, 2, 64), T(128, 256, 2, 4, 2, 64),
    T(64, 128, 2, 2, 2, 64),  GemmTile::G256,           GemmTile::PERSIST,        T(128, 128, 4, 2, 4, 32),
    T(128, 128, 4, 2, 3, 32), T(128, 64, 2, 2, 4, 32),  T(256, 128, 4, 2, 3, 32), T(256, 128, 4, 2, 4, 32),
    RING(256, 128, 4, 2, 3, 32), RING(128, 128, 4, 2, 4, 32), RING(128, 128, 4, 2, 2, 64), RING(256, 256, 4, 2, 3, 32),
    RING(256, 128, 4, 2, 2, 64), T(128, 64, 4, 2, 2, 64), T(64, 128, 2, 4, 2, 64),  T(128, 64, 4, 2, 3, 64),
    T(64, 128, 2, 4, 3, 64)};

bool out16(int epi) { return epi == EPI_BF16 || epi == EPI_GELU_BF16; }
bool dense_epi(int epi) { return out16(epi) || epi == EPI_RESID_F32 || epi == EPI_F32 || epi == EPI_POS_F32; }

// rounds of the chip's workgroup slots that `tiles` tiles per launch take, counting the concurrent stream parts
int rounds(int conc, int tiles, int slots) { return ((conc > 1 ? conc : 1) * tiles + slots - 1) / slots; }

struct Planner {
  const GemmShape& s;
  const GemmKnobs& k;
  const int cus, force;

  int tiles_m(int bm) const { return (s.M + bm - 1) / bm; }
  GemmPlan err(const char* why) const { return GemmPlan{GemmTile::NONE, 1, false, 0, why}; }
  GemmPlan with(GemmTile t, int gm_max, int ks = 1) const {
    const int tm = tiles_m(info(t).bm);
    const bool defer = ks > 1 && s.defer_reduce && s.groups == 1 && s.epi == EPI_RESID_F32 && ks <= kMaxDeferKs;
    return GemmPlan{t, ks, defer, tm < gm_max ? tm : gm_max, nullptr};
  }
  // super-tile height (tile rows walked together, column-major inside): 8 rows x all columns keeps a short-K
  // GEMM's weight slab shared per XCD; a long-K GEMM (fc2: K = 3072; the head conv: K = 6912) re-fetches its
  // large A row blocks once per column tile unless the row's column tiles run close together (gm = 4: head
  // conv 359 -> 331 us at 32 sequences, fc2 level, tests/sweep_gm_b32.sh; +0.5 % over gm = 2, ab_env.sh)
  int super_rows() const { return k.gm > 0 ? k.gm : (s.K >= 2048 ? k.gm_longk : 8); }

  // what each kernel family can run (the former launchers' guards): a plan is always launchable
  bool ok256s(bool t320) const {
    return s.N % 256 == 0 && s.K % 32 == 0 && s.K >= 64 && s.amode == A_DENSE && (t320 ? out16(s.epi) : dense_epi(s.epi));
  }
  bool ok128w() const {
    return s.N % 256 == 0 && s.K % 32 == 0 && s.K >= 32 && s.amode == A_DENSE &&
           (s.epi == EPI_RESID_F32 || s.epi == EPI_F32 || s.epi == EPI_POS_F32);
  }
  // K / BK >= NS: a tile's bias (issued after the previous epilogue) has landed before its own epilogue
  bool ok_ring(GemmTile t) const {
    const TileInfo& i = info(t);
    return s.N % i.bn == 0 && s.groups == 1 && s.amode == A_DENSE && s.K % i.bk == 0 && s.K / i.bk >= i.depth && out16(s.epi);
  }
  bool ok_persist() const { return s.N % 128 == 0 && s.groups == 1 && out16(s.epi); }

  GemmPlan g256s(bool t320) const { return with(t320 ? GemmTile::G256S_320 : GemmTile::G256S, k.gm256); }
  GemmPlan g128w() const { return with(GemmTile::G128W, super_rows()); }
  // a gemm_kernel tile; the conv gather walks 64-channel K-tiles and has the ReLU epilogues only
  GemmPlan kernel(GemmTile t) const {
    if (!(info(t).modes & (s.split ? 2 : 1))) return err("tile not built for this precision");
    if (s.amode == A_CONV3) {
      if (info(t).bk != 64 || (s.epi != EPI_RELU_BF16 && s.epi != EPI_RELU_F32))
        return err("the 3x3 conv gather needs a 64-deep tile and a ReLU epilogue");
    } else if (!dense_epi(s.epi)) {
      return err("no dense kernel with this epilogue (ReLU epilogues: conv, or a split-K shape)");
    }
    return with(t, super_rows());
  }

  // a pinned tile: false where the pin does not apply to this shape (the rules decide)
  bool pinned(GemmTile t, GemmPlan* p) const {
    switch (t) {
      case GemmTile::NONE: return false;
      case GemmTile::G256S: if (!ok256s(false)) return false; *p = g256s(false); return true;
      case GemmTile::G256:
        if (s.N % 256) return false;
        *p = dense_epi(s.epi) ? with(t, 4) : err("gemm256 has no such epilogue");
        return true;
      case GemmTile::PERSIST: if (!ok_persist()) return false; *p = with(t, 8); return true;
      default:
        if (t >= RING(256, 128, 4, 2, 3, 32) && t <= RING(256, 128, 4, 2, 2, 64)) {
          if (!ok_ring(t)) return false;
          *p = with(t, 8);
        } else {
          *p = kernel(t);
        }
        return true;
    }
  }

  GemmPlan plan() const {
    if (s.epi < 0 || s.epi > EPI_POS_F32) return err("unknown epilogue");
    GemmPlan p;
    const bool dense = s.amode == A_DENSE;
    if (s.split) {
      // tuning override of the f16x3 tile (MMT_SPLIT_CFG), dense A only
      if (k.split_cfg >= 0 && k.split_cfg < 20 && dense && (k.split_cfg != 15 || s.N >= 2048) &&
          pinned(kSplitCfg[k.split_cfg], &p))
        return p;
      // f16x3: the 8-phase 256 x 256 kernel where there are enough 256-wide column tiles (qkv, fc1: 250-300
      // TF/s vs 240-250 for the 2-barrier 128 x 128 kernel); N = 768 stays on 128-row tiles (3 column tiles of
      // 256 leave most CUs idle): MMT_256S_MIN, below.
      // The residual GEMMs (fc2, proj: N = 768) on the eight-phase kernel where its 256 x 256 tiles fill at least three
      // quarters of a round of the chip, counting the concurrent stream part: OSTrack-384's 720- and 548-token layers
      // (270 / 210 tiles; OSTrack 2 987 -> 3 045 frames/s with fc2 and proj at a full round, r06_ab_resid_256s.txt).  The
      // ViT layers' 120 tiles stay on the 128-row kernels: fc2 there lost 10 % (four times the work per tile lengthens
      // each stream half's chain).  MMT_RESID_256S: 0 never, 2 always (tuning)
      const int n256 = s.N / 256, conc = s.conc > 1 ? s.conc : 1;
      if (k.resid_256s && s.epi == EPI_RESID_F32 && s.groups == 1 && s.N % 256 == 0 &&
          (k.resid_256s == 2 || 4 * conc * tiles_m(256) * n256 >= 3 * cus) && ok256s(false))
        return g256s(false);
      // 320 x 256 tiles where they take fewer rounds of the one-workgroup-per-CU slots than 256 x 256 ones by more than
      // their 1.25x work per tile, counting the concurrent stream part (qkv of the 244-token layers, fc1 of the
      // 190-token ones at 2 x 16 sequences: two rounds -> one; OSTrack-384 2 914 -> 3 000 frames/s, r06_ab_t320_ostrack.txt;
      // ties, 5 rounds of 320-row tiles for 5 of 256-row ones, measured -0.6 %).  MMT_T320: 0 never, 1 the rule, 2 always
      // (tuning)
      bool use320 = k.t320 && s.groups == 1 && out16(s.epi) &&
                    (k.t320 == 2 || 5 * rounds(conc, tiles_m(320) * n256, cus) < 4 * rounds(conc, tiles_m(256) * n256, cus));
      // 128 x 256 two-group tiles (gemm128w_kernel) for the fp32-output N = 768 GEMMs where the 256-row kernel's tiles
      // would leave most CUs idle.  MMT_W256: 0 never, 1 the rule, 2 always (tuning); mmt_gemm_force_config(128) pins
      // it; any other pin only switches the rule off
      if (force == 128 && ok128w()) return g128w();
      if (k.w256 && force < 0 && s.epi == EPI_RESID_F32 && s.groups == 1 && s.N % 256 == 0 && s.N < 2048) {
        // the rule: its tiles fill at least 90 % of one round of the one-workgroup-per-CU slots, counting the concurrent
        // stream part, where 128 x 128 tiles would take two rounds or more
        const int tw = conc * tiles_m(128) * n256;
        if ((k.w256 == 2 || (tw <= cus && 10 * tw >= 9 * cus && rounds(conc, tiles_m(128) * (s.N / 128), cus) >= 2)) && ok128w())
          return g128w();
      }
      const bool forced = force == 320 || force == 256;   // tests: pin the tile (any tile count)
      if (forced) use320 = force == 320 && out16(s.epi);  // 320 with an fp32 epilogue: the 256-row tile
      if ((s.N >= 2048 || forced) && (tiles_m(256) * n256 * s.groups >= k.t256_min || forced) && ok256s(use320))
        return g256s(use320);
    } else if (force >= 0 && force < 25 && dense && pinned(kForceCfg[force], &p)) {
      return p;
    }
    // Measured on the path's shapes (tests/bench_gemm.py, MI355X): 128x128 tiles with 8 waves (32x64
    // per wave) and a 2-deep LDS ring (64 KB, two workgroups per CU, so one tile's prologue/epilogue
    // overlaps the other's MFMAs) beat 256x128 / 256x256 / 3-deep rings on every K=768/3072 GEMM.
    const int target = 200;   // aim for at least ~one tile per CU of the 256
    const int t128 = tiles_m(128), t64 = tiles_m(64);
    // bf16-output GEMMs with several 128 x 128 tiles per workgroup slot: the persistent kernel (the next
    // tile's first K-tile loads under the current tile's tail)
    if (!s.split && k.persist_min > 0 && dense && ok_persist() && t128 * (s.N / 128) >= k.persist_min * 2 * cus)
      return with(GemmTile::PERSIST, 8);
    const int t128n = t128 * (s.N / 128) * s.groups;
    // f16x3 N = 768 GEMMs (proj, fc2, patch): 128 x 128 tiles from 128 tiles up -- every M of the path in a
    // two-stream half (the 128 x 64 tiles that suit bf16's under-filled launches are slower here: the split
    // GEMMs are 3x longer per tile, and the other half fills the tail; from 64 tiles: +1.8 % vs 200 and +1.9 %
    // more vs 128 once the head convs (grouped, N = 3 x 128) take it too, sweep_t128.sh / ab_env.sh); a short
    // K streams 32-deep K-tiles (proj 51 -> 48 us, patch 98 -> 85 us at 32 sequences, tests/sweep_split_cfg_b32.sh),
    // fc2's K = 3072 keeps 64-deep ones (144 -> 135 us)
    // (not for one sequence's few rows: fc1 at M = 320 keeps 240 64 x 64 workgroups instead of 72; the head's implicit
    // 3x3 conv, A_CONV3 with K = 6912, gathers 64-channel K-tiles)
    if (s.split && s.N % 128 == 0 && t128n >= k.split_t128 && t128 >= 8) {
      // 128 x 192 tiles where all of them fit one round of the chip's one-workgroup-per-CU slots and 128 x 128 tiles
      // would take two or more, counting the launches of the other stream parts that run beside this one (conc):
      // the head's conv1 at 2 x 16 sequences (256 tiles in one round instead of 384: 287 -> 196 us alone), fc2 / proj
      // after candidate elimination (fc2 123.6 -> 107.4 us per launch; the line +0.8 %, profiles/r05_ab_t192.txt).
      // Where the 192-wide tiles take several rounds too (OSTrack-384's long layers: 3 against 5) they lost 1 %, so
      // a one-round fit is the rule.  MMT_T192: 0 never, 2 always (tuning)
      if (k.t192 && s.N % 192 == 0 && s.groups == 1 && (s.amode == A_CONV3 || s.K % 64 == 0) &&
          (k.t192 == 2 || (rounds(s.conc, t128 * (s.N / 192), cus) == 1 && rounds(s.conc, t128 * (s.N / 128), cus) >= 2)))
        return kernel(T(128, 192, 4, 2, 2, 64));
      // (the N = 768 GEMMs -- proj, patch -- take the register-pipelined 64-deep tile since it exists: proj at one
      // half's rows 31 -> 25 us (5 120 rows) .. 27 -> 22 us (2 432), tests/r3_run33.sh; the wide qkv / fc1 fallbacks
      // keep the 32-deep ring, level or better there)
      return kernel(s.K <= 1024 && dense && s.N > 768 ? T(128, 128, 4, 2, 2, 32) : T(128, 128, 4, 2, 2, 64));
    }
    // a little under one 128 x 128 tile per CU (the N = 768 GEMMs of the CE-pruned layers): 128 x 64 tiles
    // with 8 waves put two workgroups on most CUs (fc2 at M = 4896: 41.4 -> 34.8 us)
    if (s.N % 128 == 0 && t128n >= target) return kernel(t128n < cus ? T(128, 64, 4, 2, 2, 64) : T(128, 128, 4, 2, 2, 64));
    if (s.N % 64 == 0) {
      if (t128 * (s.N / 64) * s.groups >= target) return kernel(T(128, 64, 2, 2, 2, 64));
      const GemmTile deep = s.split ? T(64, 64, 4, 2, 3, 64) : T(64, 64, 4, 2, 4, 64);
      // few 64 x 64 tiles and a long K (small batches): split K over workgroups (fp32 partials in the
      // workspace, fixed-order reduction with the epilogue), at least 4 K-tiles per split
      // (100, not 128: qkv of the 129..192-row CE layers at one sequence -- 108 tiles -- runs unsplit without its
      // reduce launch, 1092 -> 1100 frames/s, profiles/r05_ab_splitk_tiles_b1.txt)
      const int tiles = t64 * (s.N / 64) * s.groups, nk = s.K / 64;
      if (s.has_ws && s.ws_elems > 0 && tiles < k.splitk_tiles && k.splitk_minkt > 0 && nk >= 2 * k.splitk_minkt) {
        // slices per tile rounded DOWN, so the slices of every tile run in one round of workgroups (fc2 at one
        // sequence: 60 tiles x 4 = 240 workgroups of 768-deep slices beat 300 of 614 that take two rounds on 44
        // CUs; 823 -> 906 frames/s, round 2).  64 x 64 few-tile GEMMs with 8 waves (16 x 32 each): twice
        // the waves issuing each K-tile's LDS-DMA loads -- at one sequence these GEMMs are bound by what a CU can take in
        // (one tile per CU, ~400 KB of hi + lo operands at ~45 GB/s), 906 -> 929 frames/s against 4 waves
        // (tests/few_w8_ab.sh)
        int ks = k.splitk_target / tiles;
        ks = ks < nk / k.splitk_minkt ? ks : nk / k.splitk_minkt;
        ks = ks < k.splitk_max ? ks : k.splitk_max;
        while (ks > 1 && (int64_t)ks * s.groups * s.M * s.N > s.ws_elems) --ks;
        // f16x3: a 3-deep ring (96 KB of LDS) beat 4-deep at one sequence (tests/sweep_ring_b1.sh); the slices'
        // partial sums and the reduce launch serve every epilogue, dense or conv
        if (ks > 1) return with(deep, 8, ks);
      }
      // few tiles (small batches): each workgroup walks the whole K serially, so keep K-tiles in flight
      // (bf16: 4-deep LDS ring, an 8-deep one measured no better at M = 320; f16x3: 3-deep, qkv 17.3 ->
      // 15.4 us and fc1 16.8 -> 16.5 us at one sequence, tests/sweep_ring_b1.sh)
      return kernel(s.K >= 6 * 64 ? deep : T(64, 64, 2, 2, 2, 64));
    }
    return kernel(t64 * (s.N / 32) * s.groups >= target ? T(64, 32, 4, 1, 2, 64) : T(32, 32, 2, 1, 2, 64));
  }
};

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

}  // namespace

const char* gemm_tile_name(GemmTile t) { return info(t).name; }

GemmKnobs gemm_knobs_from_env() {
  GemmKnobs k;
#define KNOB(field, NAME) k.field = env_int("MMT_" NAME, k.field)
  KNOB(split_cfg, "SPLIT_CFG"); KNOB(t256_min, "256S_MIN"); KNOB(resid_256s, "RESID_256S"); KNOB(t320, "T320");
  KNOB(w256, "W256"); KNOB(persist_min, "PERSIST_MIN"); KNOB(split_t128, "SPLIT_T128"); KNOB(t192, "T192");
  KNOB(splitk_tiles, "SPLITK_TILES"); KNOB(splitk_target, "SPLITK_TARGET"); KNOB(splitk_minkt, "SPLITK_MINKT");
  KNOB(splitk_max, "SPLITK_MAX"); KNOB(gm, "GM"); KNOB(gm_longk, "GM_LONGK"); KNOB(gm256, "GM256");
#undef KNOB
  return k;
}

GemmPlan gemm_plan(const GemmShape& s, const GemmKnobs& k, int num_cus, int force_cfg) {
  return Planner{s, k, num_cus, force_cfg}.plan();
}

}  // namespace mmt
