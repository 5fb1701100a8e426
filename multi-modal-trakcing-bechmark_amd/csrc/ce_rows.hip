// Candidate-elimination probabilities over a SET of template rows (generate_mask_cond's ALL / CTR_REC / GT_BOX
// masks, ce_utils.py:15-65; attn_blocks.py:44-53), gfx950:
//
//   prob[b][h][j] = 1 / nrows[b] * sum_{r in rows[b]} softmax_k(q_r . k_k * 64^-0.5)[lens_t + j]
//
// in the layout attention's single-row export writes (AttnArgs::ce_prob), so ce_select / ce_layernorm read it
// unchanged.  It runs after attention on the same qkv buffer and recomputes the template rows' logits: Lz / N of
// attention's QK work, no PV.
//
// One workgroup = one (sequence, head), four waves; wave w takes the 16-row blocks w, w + 4, ... of the sequence's
// compact row list, one block per round.  A round streams the K tiles (64 keys, hi + lo planes in the parity mode:
// the whole K of N = 720 would be 184 KB) through ONE LDS slot twice:
//   pass 1, every key tile:        the online (max, sum) of the wave's 16 rows, nothing else kept;
//   pass 2, the search-key tiles:  the logits again, p = exp((s - m) qks) / l with the full-length m and l, the 16
//                                  rows of the block summed by the fixed DPP steps of row16_sum, added into the
//                                  wave's own [N - lens_t] fp32 accumulator in LDS.
// Logits are formed swapped (S^T = K Q^T, v_mfma_f32_16x16x32) exactly as attn_kernel forms them -- a lane holds 16
// keys of ONE row -- with its three-product f16x3 sum or its bf16 product, so m and l are attention's.  After the
// last round the four accumulators are added in wave order and divided by nrows.  No atomics: a result depends only
// on the sequence's own rows and list, not on B or on its place in the batch.
//
// LDS hazards: the K slot is rewritten every step between two fences, each an explicit s_waitcnt lgkmcnt(0) and a
// workgroup barrier (every wave past the previous tile's reads; the new tile visible); a wave's accumulator is
// touched by that wave alone until the fence before the final sum.
#include "kernels.h"

namespace mmt {

namespace {

constexpr int KB = 64;            // keys per LDS tile
constexpr int CE_WAVES = 4;
constexpr int CE_LS_MAX = 1024;   // search keys per sequence (N <= 1024)

// byte offset of 16-B chunk c of row r in a [64][64] 16-bit tile (128-B rows, chunk XOR row: attention.hip)
__device__ __forceinline__ int tile_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }

// this wave's LDS reads and writes have completed, then the workgroup barrier
__device__ __forceinline__ void lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

template <bool SPLIT>
__global__ __launch_bounds__(CE_WAVES * 64) void ce_rows_kernel(const CeRowsArgs a) {
  constexpr int NH = SPLIT ? 2 : 1;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[NH][KB * 64];
  __shared__ float acc[CE_WAVES][CE_LS_MAX];

  const int bh = blockIdx.x, b = bh / a.heads, h = bh - b * a.heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, qc = lane & 15;
  const int N = a.N, Lt = a.lens_t, Ls = N - Lt, Cd = 64 * a.heads, C3 = 3 * Cd;
  const bf16_t* base = a.qkv + (int64_t)b * N * C3;
  const bf16_t* base_lo = SPLIT ? a.qkv_lo + (int64_t)b * N * C3 : nullptr;
  const int* rows = a.rows + (int64_t)b * a.pitch;
  // (the launchers' callers validate the lists; clamped all the same, so no list can index past the template)
  const int nr = __builtin_amdgcn_readfirstlane(min(max(a.nrows[b], 0), min(Lt, a.pitch)));
  const int nblk = (nr + 15) >> 4, rounds = (nblk + CE_WAVES - 1) / CE_WAVES;
  const int T1 = (N + KB - 1) / KB;   // pass 1: every key tile
  const int t2 = Lt / KB;             // pass 2 starts at the first tile holding a search key (lens_t < N)
  const int TS = T1 + (T1 - t2);      // steps per round
  auto tile_kb = [&](int u) { return (u < T1 ? u : t2 + (u - T1)) * KB; };

  for (int j = lane; j < Ls; j += 64) acc[wave][j] = 0.f;

  // K staging through registers, software-pipelined: the next step's 16-B chunks are loaded while this step's tile
  // is multiplied
  constexpr int NCHT = NH * KB * 8 / (CE_WAVES * 64);
  uint4 kreg[NCHT];
  auto fetch = [&](int kb) {
#pragma unroll
    for (int i = 0; i < NCHT; ++i) {
      const int q = tid + i * (CE_WAVES * 64);
      const int hl = q / (KB * 8), qq = q - hl * (KB * 8);
      const int r = qq >> 3, c = qq & 7, key = kb + r;
      kreg[i] = make_uint4(0, 0, 0, 0);   // keys past N: zeros (masked in pass 1, not accumulated in pass 2)
      if (key < N) kreg[i] = *reinterpret_cast<const uint4*>((hl ? base_lo : base) + (int64_t)key * C3 + Cd + h * 64 + c * 8);
    }
  };

  const float qks = SPLIT ? a.qk_inv : 1.0f;   // the logits' scale (f16x3: accumulator units, attention.hip)
  const float lg = qks * 1.44269504f;
  bf16x8 qf[NH][2];
  float m = -INFINITY, l = 0.f;
  bool valid = false;

  if (rounds > 0) fetch(0);
#pragma unroll 1
  for (int it = 0; it < rounds; ++it) {
    const int rb = wave + CE_WAVES * it;   // this wave's row block of the round (wave-uniform)
#pragma unroll 1
    for (int u = 0; u < TS; ++u) {
      const int kb = tile_kb(u);
      lds_fence();       // every wave is past its reads of the previous tile
#pragma unroll
      for (int i = 0; i < NCHT; ++i) {
        const int q = tid + i * (CE_WAVES * 64);
        const int hl = q / (KB * 8), qq = q - hl * (KB * 8);
        *reinterpret_cast<uint4*>(reinterpret_cast<char*>(Ks[hl]) + tile_off(qq >> 3, qq & 7)) = kreg[i];
      }
      lds_fence();       // the tile is visible to every wave
      if (u + 1 < TS) fetch(tile_kb(u + 1));
      else if (it + 1 < rounds) fetch(0);
      if (rb >= nblk) continue;   // no block left for this wave: it stages and meets the barriers only

      if (u == 0) {
        // the block's 16 rows; a last block's padding rows load zeros and are weighted out below (a zero row's
        // softmax is uniform, not zero)
        const int qi = rb * 16 + qc;
        valid = qi < nr;
        const int row = valid ? min(max(rows[qi], 0), Lt - 1) : 0;
#pragma unroll
        for (int hl = 0; hl < NH; ++hl)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            qf[hl][s] = bf16x8{};
            if (valid) {
              const bf16x8 qv =
                  *reinterpret_cast<const bf16x8*>((hl ? base_lo : base) + (int64_t)row * C3 + h * 64 + 32 * s + 8 * g);
              if (SPLIT) {   // f16x3: the 1/8 is folded into qk_inv
                qf[hl][s] = qv;
              } else {       // bf16: 2^-3 folded into Q, exact (attention.hip)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[hl][s][e] = (__bf16)((float)qv[e] * 0.125f);
              }
            }
          }
        m = -INFINITY;
        l = 0.f;
      }

      // S^T tile: lane (g, qc) holds keys kb + 16 t + 4 g + r of row qc
      f32x4 sc[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int r = 16 * t + qc, c = 4 * s + g;
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Ks[0]) + tile_off(r, c));
          sc[t] = mfma16<SPLIT>(kf, qf[0][s], sc[t]);
          if (SPLIT) {
            const bf16x8 kl = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Ks[NH - 1]) + tile_off(r, c));
            sc[t] = mfma16<SPLIT>(kl, qf[0][s], sc[t]);
            sc[t] = mfma16<SPLIT>(kf, qf[NH - 1][s], sc[t]);
          }
        }
      }

      if (u < T1) {
        // pass 1: online max and sum, attn_kernel's arithmetic
        if (kb + KB > N) {
          const int lim = N - kb - 4 * g;
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (16 * t + r >= lim) sc[t][r] = -INFINITY;
        }
        float bmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) bmax = fmaxf(bmax, sc[t][r]);
        bmax = xmax16(bmax);
        bmax = xmax32(bmax);
        const float mnew = fmaxf(m, bmax);
        const float alpha = __expf((m - mnew) * qks);
        const float ml2 = mnew * lg;
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) psum += __builtin_amdgcn_exp2f(fmaf(sc[t][r], lg, -ml2));
        psum = xsum16(psum, psum);
        psum = xsum32(psum, psum);
        l = l * alpha + psum;
        m = mnew;
      } else {
        // pass 2: the block's probability column sums of this tile.  Value (t, r) summed over the 16 rows lands in
        // lane qc = 4 t + r of each 16-lane group, whose key is then kb + 16 (qc >> 2) + 4 g + (qc & 3)
        float mine = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = valid ? __expf((sc[t][r] - m) * qks) / l : 0.f;
            const float ps = row16_sum(p);
            if (qc == 4 * t + r) mine = ps;
          }
        const int key = kb + 16 * (qc >> 2) + 4 * g + (qc & 3);
        if (key >= Lt && key < N) acc[wave][key - Lt] += mine;
      }
    }
  }

  lds_fence();   // every wave's accumulator is complete
  float* dst = a.prob + ((int64_t)b * a.heads + h) * Ls;
  for (int j = tid; j < Ls; j += CE_WAVES * 64) {
    float v = acc[0][j];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) v += acc[w][j];   // wave order
    dst[j] = nr > 0 ? v / (float)nr : 0.f;
  }
}

}  // namespace

void ce_rows(const CeRowsArgs& a, hipStream_t s) {
  if (a.qkv_lo)
    hipLaunchKernelGGL((ce_rows_kernel<true>), dim3(a.B * a.heads), dim3(CE_WAVES * 64), 0, s, a);
  else
    hipLaunchKernelGGL((ce_rows_kernel<false>), dim3(a.B * a.heads), dim3(CE_WAVES * 64), 0, s, a);
}

}  // namespace mmt
