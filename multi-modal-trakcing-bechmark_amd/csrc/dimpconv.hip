// mfDiMP / DeT-DiMP ResNet-50 convolutions on the fp16 matrix cores at fp32-faithful precision ("f16x3"),
// gfx950.  The same implicit GEMM as dimpnet.hip's conv_f32_kernel (C[m][n] = sum_k A[m][k] W[n][k],
// m = output pixel, n = output channel, k = (ky, kx, c); activations NHWC fp32, weights [Cout][kh][kw][Cin]
// with BN folded on the host), but every product is carried as the fp16 pair of a power-of-two range-scaled
// value (common.h): acc += Wh*Ah + Wl*Ah + Wh*Al on v_mfma_f32_16x16x32_f16 -- 22-bit operands and fp32
// accumulation, the reference's fp32 arithmetic to within 2^-22 per product, at 5.3x the fp32 matrix peak
// (833 vs 157 TF/s of algorithmic FLOPs).
//
// Range scales.  Weights: s_w = 2^(14 - ceil(log2 max|w|)), split on the host.  Activations: each conv's
// epilogue folds max|y| of its output into 64 sharded max words (one per 128-B line, agent-scope atomic max
// of the float bits -- a wave's maximum per atomic), and the consuming conv reads the 64 words, takes
// s_a = 2^(14 - ceil(log2 max)) and splits its input on the fly while staging it into LDS (loads through
// registers); so |v s_a| <= 2^14 for every element, and an element keeps full 22-bit precision down to
// 2^-17 of its tensor's maximum (below that its absolute error is under 2^-38 of the maximum).  Image
// inputs (normalised pixels, |v| <= 2.64) use the static scale 2^12.
//
// Tile: 128 output pixels x BN (64 / 128) output channels, 8 waves (4 x 2, 32 x BN/2 each), K-tiles of 32:
// FAST = 32 channels of one tap (Cin % 32 == 0); STEM = 8 taps x 4 channels (Cin = 3, weights padded to 4
// channels per tap and to whole K-tiles).  Two LDS stages (hi / lo images of A and W, 16-B chunks XOR-swizzled
// as gemm.hip's BK = 32 tiles, so fragment reads are conflict-free ds_read_b128) and two register sets: the
// global loads of K-tile k + 2 are issued before K-tile k is multiplied.  The MFMA is issued W x A, so a lane
// ends with 4 consecutive output channels of one pixel (16-B NHWC stores).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/mmtrack.h"
#include "common.h"
#include "conv_plan.h"

namespace mmt {

constexpr int kMaxShards = 64, kShardStride = 32;   // sharded max words: 64 x 128-B lines per tensor


struct ConvGroupArgs {            // one convolution of a grouped launch (the RGB / aux backbones' twin layers)
  const float* x;                 // [N][H][W][Cin] fp32
  const uint16_t* wh;             // [Cout][Kp] fp16 halves of w * s_w
  const uint16_t* wl;
  const float* bias;              // [Cout] or null
  const float* resid;             // [M][Cout] or null
  float* y;                       // [M][Cout]
  const float* xmax;              // sharded max|x| words of the input, or null: xscale
  float* ymax;                    // sharded max|y| words of the output (accumulated), or null
  float xscale;                   // static input scale (power of two) when xmax is null
  float inv_w;                    // 1 / s_w
  int flags;
  const float* x2;                // Cin2 > 0: the block input the fused downsample reads ([N][H2][W2][Cin2])
  const float* x2max;             // its sharded max words, or null: x2scale
  float x2scale;
};

struct ConvF16Args {
  ConvGroupArgs g[kMaxGroups];
  float* part;                    // split-K partials [ks][G][M][Cout] (ks > 1)
  int N, H, W, Cin, Cout, kh, kw, stride, pad, Ho, Wo, Kp, ks;
  // xcd_order and staged_epi (below): the host sets both to 1.  The fields and the kernel branches that read them
  // stay so that every kernel's argument layout, and with it its code, is what was measured
  int xcd_order;                  // conv_f16x3_deep_kernel: XCD-aware tile order (else M tiles fastest)
  // a downsample fused into a 1 x 1 conv3 (conv_f16x3_deep_kernel only): K-tiles from Cin / 32 on read x2 at
  // output pixel (oy, ox) * stride2; 0: none
  int Cin2, H2, W2, stride2;
  int staged_epi;                 // conv_f16x3_deep_kernel: the LDS-staged epilogue
};

__device__ __forceinline__ int cswz(int r, int c) { return r * 32 + ((c ^ ((r >> 2) & 2)) << 3); }   // gemm.hip swzk<32>

__device__ __forceinline__ float pow2_scale(float m) {   // 2^(14 - ceil(log2 m)), m > 0
  int e;
  const float f = frexpf(m, &e);   // m = f 2^e, f in [0.5, 1)
  const int c = f == 0.5f ? e - 1 : e;
  return ldexpf(1.0f, 14 - c);
}

__device__ __forceinline__ ConvGroupArgs pick_group(const ConvF16Args& a, int grp) {
  return grp ? a.g[1] : a.g[0];   // a select, not a dynamic index (which would copy the arguments to scratch)
}

// the epilogue arithmetic shared by every conv kernel, spelled out (contraction off, the bias added by an explicit
// fused multiply-add) so that each kernel rounds the same way whatever the compiler would contract:
// conv_lin = acc / (s_w s_a) + bias; conv_tail = + residual, ReLU, the backbones' running max, store
__device__ __forceinline__ f32x4 conv_lin(const ConvGroupArgs& g, const f32x4& acc, float inv, int no) {
#pragma clang fp contract(off)
  if (!g.bias) return acc * inv;
  const float4 b = *reinterpret_cast<const float4*>(g.bias + no);
  return f32x4{__builtin_fmaf(acc[0], inv, b.x), __builtin_fmaf(acc[1], inv, b.y), __builtin_fmaf(acc[2], inv, b.z),
               __builtin_fmaf(acc[3], inv, b.w)};
}
__device__ __forceinline__ f32x4 conv_tail(const ConvGroupArgs& g, f32x4 v, int64_t mo, int no, int Cout) {
#pragma clang fp contract(off)
  if (g.resid) {
    const float4 r = *reinterpret_cast<const float4*>(g.resid + mo * Cout + no);
    v += f32x4{r.x, r.y, r.z, r.w};
  }
  if (g.flags & MMT_CONV_RELU)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  float4* dst = reinterpret_cast<float4*>(g.y + mo * Cout + no);
  if (g.flags & MMT_CONV_MAX) {
    const float4 o = *dst;   // torch.max(color, depth) (dimpnet.py:103)
    v = f32x4{fmaxf(o.x, v[0]), fmaxf(o.y, v[1]), fmaxf(o.z, v[2]), fmaxf(o.w, v[3])};
  }
  *dst = make_float4(v[0], v[1], v[2], v[3]);
  return v;
}
// the split-K path: v = the slices' sum (each slice already scaled) + bias, then the tail
__device__ __forceinline__ f32x4 conv_out(const ConvGroupArgs& g, f32x4 v, int64_t mo, int no, int Cout) {
#pragma clang fp contract(off)
  if (g.bias) {
    const float4 b = *reinterpret_cast<const float4*>(g.bias + no);
    v += f32x4{b.x, b.y, b.z, b.w};
  }
  return conv_tail(g, v, mo, no, Cout);
}

// a wave's FM x FN output fragments (rows mo[i] where mv[i], columns nb + 16 j .. + 3) through conv_out's arithmetic
// in its order, the operands requested together before any is used (the FN bias groups, every fragment's residual)
// through raw buffer loads -- an absent operand is a zero-sized buffer, a row past the map an out-of-range offset, both
// read zeros -- so the FM x FN residual round trips overlap instead of each waiting in place (the K loop's registers
// are dead by now: no register cost); returns the lane's max |y|.  rows = the launch's output rows (M)
template <int FM, int FN>
__device__ __forceinline__ float conv_store_tile(const ConvGroupArgs& g, const f32x4 (&acc)[FM][FN], float inv,
                                                 const int64_t (&mo)[FM], const bool (&mv)[FM], int nb, int Cout,
                                                 int64_t rows) {
#pragma clang fp contract(off)
  if (rows * Cout * 4 >= ((int64_t)1 << 31)) {   // past a 32-bit buffer offset: conv_tail's plain loads
    float ymx = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if (!mv[i]) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const f32x4 v = conv_tail(g, conv_lin(g, acc[i][j], inv, nb + 16 * j), mo[i], nb + 16 * j, Cout);
#pragma unroll
        for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
      }
    }
    return ymx;
  }
  const rsrc_t rR = make_rsrc(g.resid, g.resid ? rows * Cout * 4 : 0);
  const rsrc_t rB = make_rsrc(g.bias, g.bias ? (int64_t)Cout * 4 : 0);
  f32x4 bv[FN], rv[FM][FN];
#pragma unroll
  for (int j = 0; j < FN; ++j)
    bv[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rB, (uint32_t)((nb + 16 * j) * 4), 0, 0));
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const uint32_t vo = mv[i] ? (uint32_t)((mo[i] * Cout + nb + 16 * j) * 4) : kBufOob;
      rv[i][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rR, vo, 0, 0));
    }
  float ymx = 0.f;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    if (!mv[i]) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      f32x4 v = acc[i][j] * inv;
      if (g.bias)
        v = f32x4{__builtin_fmaf(acc[i][j][0], inv, bv[j][0]), __builtin_fmaf(acc[i][j][1], inv, bv[j][1]),
                  __builtin_fmaf(acc[i][j][2], inv, bv[j][2]), __builtin_fmaf(acc[i][j][3], inv, bv[j][3])};
      if (g.resid) v += rv[i][j];
      if (g.flags & MMT_CONV_RELU)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      float4* dst = reinterpret_cast<float4*>(g.y + mo[i] * Cout + nb + 16 * j);
      if (g.flags & MMT_CONV_MAX) {
        const float4 o = *dst;   // torch.max(color, depth) (dimpnet.py:103)
        v = f32x4{fmaxf(o.x, v[0]), fmaxf(o.y, v[1]), fmaxf(o.z, v[2]), fmaxf(o.w, v[3])};
      }
      *dst = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
      for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
    }
  }
  return ymx;
}

// conv_store_tile through the LDS: the workgroup's 128-pixel x BN tile (8 waves: 4 row quarters x 2 column halves,
// FM = 2) goes to `lds` (>= 128 x BN floats; 16-B chunk q of row r at q ^ (r & 7)) as conv_lin's values, then every
// thread takes whole 16-B row chunks -- 32 lanes cover a pixel's 512 B of a 128-wide tile -- adds the residual,
// ReLU and the merge and stores them: full 128-B lines for the output and the residual instead of a fragment's 16
// rows x 16 B per wave instruction (the HBM-bound 1 x 1 convs of layers 1 / 2 spend most of their time here).  Same
// arithmetic, same order as conv_store_tile, so the same bits.  Rows r valid below row_end (row0 + r = the pixel).
template <int FN, int BN>
__device__ __forceinline__ float conv_store_tile_staged(const ConvGroupArgs& g, const f32x4 (&acc)[2][FN], float inv,
                                                        float* lds, int wm, int wn, int lane, int64_t row0,
                                                        int64_t row_end, int n0, int Cout, int64_t rows) {
#pragma clang fp contract(off)
  constexpr int WN = BN / 2, NCH = BN / 4, PER = 128 * NCH / 512;
  const int li = lane & 15, lk = lane >> 4, t = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every LDS-DMA of the K loop has landed
  __syncthreads();                                   // and every wave is past its last fragment read
  const rsrc_t rB = make_rsrc(g.bias, g.bias ? (int64_t)Cout * 4 : 0);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int c = wn * WN + j * 16 + 4 * lk;
    const f32x4 bv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rB, (uint32_t)((n0 + c) * 4), 0, 0));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = wm * 32 + i * 16 + li;
      f32x4 v = acc[i][j] * inv;
      if (g.bias)
        v = f32x4{__builtin_fmaf(acc[i][j][0], inv, bv[0]), __builtin_fmaf(acc[i][j][1], inv, bv[1]),
                  __builtin_fmaf(acc[i][j][2], inv, bv[2]), __builtin_fmaf(acc[i][j][3], inv, bv[3])};
      // (| for +: the row base is a multiple of BN, the chunk offset below BN; spelled as one index, so the address
      // code does not depend on what the compiler knows of `lds` at its single call site)
      *reinterpret_cast<f32x4*>(lds + (r * BN | (((c >> 2) ^ (r & 7)) << 2))) = v;
    }
  }
  __syncthreads();
  const rsrc_t rR = make_rsrc(g.resid, g.resid ? rows * Cout * 4 : 0);
  const rsrc_t rY = make_rsrc(g.y, rows * Cout * 4);
  const bool mx = g.flags & MMT_CONV_MAX;
  constexpr int GRP = PER < 4 ? PER : 4;   // residual chunks requested together (registers: 4 x 4 per thread)
  float ymx = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < PER; k0 += GRP) {
    f32x4 res[GRP];
#pragma unroll
    for (int k = 0; k < GRP; ++k) {
      const int idx = t + 512 * (k0 + k), r = idx / NCH, q = idx - r * NCH;
      const uint32_t off = row0 + r < row_end ? (uint32_t)(((row0 + r) * Cout + n0 + 4 * q) * 4) : kBufOob;
      res[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rR, off, 0, 0));
    }
#pragma unroll
    for (int k = 0; k < GRP; ++k) {
      const int idx = t + 512 * (k0 + k), r = idx / NCH, q = idx - r * NCH;
      if (row0 + r >= row_end) continue;
      const uint32_t off = (uint32_t)(((row0 + r) * Cout + n0 + 4 * q) * 4);
      f32x4 v = *reinterpret_cast<const f32x4*>(lds + r * BN + ((q ^ (r & 7)) << 2));
      if (g.resid) v += res[k];
      if (g.flags & MMT_CONV_RELU)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      if (mx) {   // torch.max(color, depth) (dimpnet.py:103): the RGB map already in y
        const f32x4 o = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rY, off, 0, 0));
        v = f32x4{fmaxf(o[0], v[0]), fmaxf(o[1], v[1]), fmaxf(o[2], v[2]), fmaxf(o[3], v[3])};
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rY, off, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
    }
  }
  __syncthreads();   // the LDS is free again (the caller's max fold uses it)
  return ymx;
}

// the workgroup's max|y| into shard word blockIdx-derived: one agent-scope atomic max per workgroup (a per-wave
// atomic put ~1 300 atomics on each of the 64 words for the stem's 10 368 workgroups); every thread calls it
template <int NWAVES>
__device__ __forceinline__ void fold_max(float* ymax, float ymx, int shard, float* wmax /* LDS, NWAVES floats */) {
  ymx = wave_max(ymx);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = ymx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = wmax[0];
#pragma unroll
    for (int w = 1; w < NWAVES; ++w) m = fmaxf(m, wmax[w]);
    if (m > 0.f)
      __hip_atomic_fetch_max(reinterpret_cast<unsigned*>(ymax) + (shard % kMaxShards) * kShardStride,
                             __float_as_uint(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

typedef __attribute__((address_space(3))) void* lptr_t;

// one K-tile's activations in flight: 8 fp32 values of one output pixel (split into fp16 hi / lo on the way
// into the LDS); two named sets (no array, so nothing is indexed at run time and nothing goes to scratch)
struct ConvRegs {
  float4 a0, a1;
};

// grid (ceil(M / 128), Cout / BN, G * ks): blockIdx.z = group * ks + K slice
template <int BN, bool STEM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv_f16x3_kernel(const ConvF16Args a) {
  constexpr int BM = 128, BK = 32, NWS = 3;   // W ring depth
  constexpr int WN = BN / 2, FM = 2, FN = WN / 16;
  constexpr int NW = BN / 64;                  // W LDS-DMA pieces (16 rows x 64 B) per wave per K-tile
  constexpr int NA = STEM ? 6 : 2;             // A loads per thread per K-tile
  __shared__ __attribute__((aligned(16))) uint16_t sA[2][2][BM * BK];     // [stage][hi, lo]
  __shared__ __attribute__((aligned(16))) uint16_t sW[NWS][2][BN * BK];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int grp = blockIdx.z / a.ks, slice = blockIdx.z - grp * a.ks;
  const ConvGroupArgs g = pick_group(a, grp);
  const int M = a.N * a.Ho * a.Wo;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  // input scale: the maximum over the producer's 64 shard words (every wave forms it itself)
  float sa = g.xscale;
  if (g.xmax) {
    const float mx = wave_max(g.xmax[lane * kShardStride]);
    sa = mx > 0.f ? pow2_scale(mx) : 1.0f;
  }
  const float inv = g.inv_w / sa;

  // A load slot: row (pixel) t >> 2, K chunk t & 3 (8 values)
  const int ar = t >> 2, ac = t & 3;
  const int m = m0 + ar;
  const bool mval = m < M;
  int iy0 = 0, ix0 = 0;
  uint32_t xrow = 0;   // the pixel's image base (elements)
  if (mval) {
    const int nimg = m / (a.Ho * a.Wo);
    const int r = m - nimg * a.Ho * a.Wo;
    const int oy = r / a.Wo, ox = r - oy * a.Wo;
    iy0 = oy * a.stride - a.pad;
    ix0 = ox * a.stride - a.pad;
    xrow = (uint32_t)(nimg * a.H * a.W * a.Cin);
  }
  // operands through raw buffer loads: a tap outside the image, a row past M or a K-tile past the slice takes
  // an offset past the resource and reads zeros, so every load is issued unconditionally (a branch around a
  // load makes the compiler wait for it in place)
  const rsrc_t rX = make_rsrc(g.x, (int64_t)a.N * a.H * a.W * a.Cin * 4);
  const int nk = a.Kp / BK;
  const int kt0 = (int)((int64_t)slice * nk / a.ks), nt = (int)((int64_t)(slice + 1) * nk / a.ks) - kt0;
  const int cpt = STEM ? 1 : a.Cin / BK;   // K-tiles per tap

  auto load_a = [&](int kt, bool kv, ConvRegs& r) {   // kv false: zeros (a tile past the slice, no traffic)
    if constexpr (STEM) {
      // taps 8 kt + 2 ac, + 1: three channels each (the fourth is the weights' zero pad); a 4-channel input
      // (Cin 4: pixels padded with a zero fourth channel, mmt_image_normalize4) loads a tap as one float4
      if (a.Cin == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int tap = kt * 8 + ac * 2 + h;
          const int ky = tap / a.kw, kx = tap - ky * a.kw;
          const int iy = iy0 + ky, ix = ix0 + kx;
          const bool ok = kv && mval && tap < a.kh * a.kw && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
          const uint32_t vo = ok ? (xrow + (uint32_t)((iy * a.W + ix) * 4)) * 4 : kBufOob;
          (h ? r.a1 : r.a0) = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo, 0, 0));
        }
        return;
      }
      float v[2][3];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tap = kt * 8 + ac * 2 + h;
        const int ky = tap / a.kw, kx = tap - ky * a.kw;
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = kv && mval && tap < a.kh * a.kw && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const uint32_t vo = ok ? (xrow + (uint32_t)((iy * a.W + ix) * 3)) * 4 : kBufOob;
#pragma unroll
        for (int e = 0; e < 3; ++e)
          v[h][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rX, vo + 4 * e, 0, 0));
      }
      r.a0 = make_float4(v[0][0], v[0][1], v[0][2], 0.f);
      r.a1 = make_float4(v[1][0], v[1][1], v[1][2], 0.f);
    } else {
      const int tap = kt / cpt, c0 = (kt - tap * cpt) * BK + ac * 8;
      const int ky = tap / a.kw, kx = tap - ky * a.kw;
      const int iy = iy0 + ky, ix = ix0 + kx;
      const bool ok = kv && mval && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      const uint32_t vo = ok ? (xrow + (uint32_t)((iy * a.W + ix) * a.Cin + c0)) * 4 : kBufOob;
      r.a0 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo, 0, 0));
      r.a1 = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo + 16, 0, 0));
    }
  };
  // W by LDS-DMA (buffer_load ... lds, no VGPRs): piece p = wave * NW + j holds rows 16 (p % (BN / 16)) .. + 15
  // of image p / (BN / 16); lane writes LDS chunk lane & 3 of row lane >> 2 and loads the source chunk that the
  // cswz swizzle puts there
  // the W pieces are issued as inline asm: the compiler neither orders LDS reads behind them (it cannot tell the
  // ring stages apart and would wait for every DMA before each fragment read) nor counts them; the K loop waits
  // for them itself, and the compiler's own vmcnt waits for the A registers only ever wait longer because of them
  const u32x4 qWh = make_rsrc_words(g.wh, (int64_t)a.Cout * a.Kp * 2);
  const u32x4 qWl = make_rsrc_words(g.wl, (int64_t)a.Cout * a.Kp * 2);
  auto load_w = [&](int kt, bool kv, int st) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int p = wave * NW + j, img = p / (BN / 16), rb = p % (BN / 16);
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(lptr_t)(&sW[st][img][rb * 16 * BK]));
      const int row = rb * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 2);
      const uint32_t vo = kv ? (uint32_t)(((n0 + row) * a.Kp + c * 8) * 2) : kBufOob;
      const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)(kt * BK * 2));
      if (img)
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWl), "s"(so), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWh), "s"(so), "{m0}"(dst) : "memory");
    }
  };
  auto pack2 = [&](float x, float y, uint32_t& h, uint32_t& l) {
    uint16_t hx, lx, hy, ly;
    split_h(x * sa, hx, lx);
    split_h(y * sa, hy, ly);
    h = hx | (uint32_t)hy << 16;
    l = lx | (uint32_t)ly << 16;
  };
  auto stash = [&](const ConvRegs& r, int st) {
    uint4 hv, lv;
    pack2(r.a0.x, r.a0.y, hv.x, lv.x);
    pack2(r.a0.z, r.a0.w, hv.y, lv.y);
    pack2(r.a1.x, r.a1.y, hv.z, lv.z);
    pack2(r.a1.z, r.a1.w, hv.w, lv.w);
    *reinterpret_cast<uint4*>(&sA[st][0][cswz(ar, ac)]) = hv;
    *reinterpret_cast<uint4*>(&sA[st][1][cswz(ar, ac)]) = lv;
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int sta, int stw) {
    const int c = lane >> 4;
    bf16x8 ah[FM], al[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int row = wm * 32 + i * 16 + (lane & 15);
      ah[i] = *reinterpret_cast<const bf16x8*>(&sA[sta][0][cswz(row, c)]);
      al[i] = *reinterpret_cast<const bf16x8*>(&sA[sta][1][cswz(row, c)]);
    }
    // weight fragments one column block at a time (fewer live registers: two workgroups per CU; a dependent
    // 16x16x32 MFMA chain issues at the full rate, MI355X_MICROARCH.md); each accumulator takes Wh*Ah, Wl*Ah,
    // Wh*Al in that order
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int row = wn * WN + j * 16 + (lane & 15);
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&sW[stw][0][cswz(row, c)]);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&sW[stw][1][cswz(row, c)]);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        acc[i][j] = mfma16<true>(bh, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bl, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bh, al[i], acc[i][j]);
      }
    }
  };

  // K-tile kt0 + i: A loaded into register set i & 1 two tiles ahead and stashed (split) into LDS stage i & 1
  // one tile ahead; W DMA'd into ring stage i % 3 right after the stash of the tile before (one tile ahead).
  // Issue order per tile: A(i + 2), multiply i, stash A(i + 1) (the compiler's wait for its registers leaves
  // A(i + 2) in flight and retires W(i + 1), issued before it), W(i + 2), then the wait that leaves exactly
  // A(i + 2) and W(i + 2) in flight, and a raw s_barrier (__syncthreads() would wait for every load).  Loads
  // past the slice are zeros into stages nobody reads, so every load and stash is unconditional.
  auto tile_wait = [&]() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA + NW) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  ConvRegs r0, r1;
  load_a(kt0, true, r0);
  load_w(kt0, true, 0);
  load_a(kt0 + 1, nt > 1, r1);
  stash(r0, 0);
  load_w(kt0 + 1, nt > 1, 1);
  tile_wait();
  int sw = 0;   // i % 3
  for (int i = 0; i < nt; i += 2) {
    const int sw2 = sw == 0 ? 2 : sw - 1;   // (i + 2) % 3
    load_a(kt0 + i + 2, i + 2 < nt, r0);
    compute(0, sw);
    stash(r1, 1);
    load_w(kt0 + i + 2, i + 2 < nt, sw2);
    tile_wait();
    sw = sw == 2 ? 0 : sw + 1;
    if (i + 1 >= nt) break;
    const int sw3 = sw == 0 ? 2 : sw - 1;   // (i + 3) % 3
    load_a(kt0 + i + 3, i + 3 < nt, r1);
    compute(1, sw);
    stash(r0, 0);
    load_w(kt0 + i + 3, i + 3 < nt, sw3);
    tile_wait();
    sw = sw == 2 ? 0 : sw + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the zero-loads past the slice, before the LDS is left

  // lane holds channels n0 + wn * WN + j * 16 + 4 * (lane >> 4) + (0..3) of pixel m0 + wm * 32 + i * 16 + (lane & 15)
  const int li = lane & 15, lk = lane >> 4;
  if (a.ks > 1) {   // a K slice: its share of acc / (s_w s_a), summed in slice order by conv_splitk_reduce
    const int G = gridDim.z / a.ks;
    float* pb = a.part + ((int64_t)slice * G + grp) * M * a.Cout;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mo = m0 + wm * 32 + i * 16 + li;
      if (mo >= M) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int no = n0 + wn * WN + j * 16 + 4 * lk;
        const f32x4 v = acc[i][j] * inv;
        *reinterpret_cast<float4*>(pb + (int64_t)mo * a.Cout + no) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    return;
  }
  float ymx = 0.f;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int mo = m0 + wm * 32 + i * 16 + li;
    if (mo >= M) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int no = n0 + wn * WN + j * 16 + 4 * lk;
      const f32x4 v = conv_tail(g, conv_lin(g, acc[i][j], inv, no), mo, no, a.Cout);
#pragma unroll
      for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
    }
  }
  // (the operand stages are free: the K loop ended on a barrier after the last multiply)
  if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.y * 7 + blockIdx.z * 13, reinterpret_cast<float*>(&sA[0][0][0]));
}

// The stem (kh x kw / stride on a 4-channel image -- 3 channels padded with a zero one, mmt_image_normalize4 --
// and 64 output channels) as 2-D tiles of 16 x 16 output pixels: the tile's input patch ((16 - 1) s + kh rows x
// (16 - 1) s + kw columns, zeros outside the image) is loaded ONCE, split into fp16 hi / lo into LDS, and every
// K-tile's A fragments are read from it (a tap is 4 channels, 8 B per half); the weights of all K-tiles arrive
// by LDS-DMA alongside.  One dependent round trip per workgroup instead of one per K-tile
// (conv_f16x3_kernel<64, true>: 7 K-tiles of register-staged gathers), with the same products in the same
// order, so the output is that kernel's bit for bit.
// 16 tile rows (against 8) halve the weight re-fetch per output pixel; 79 KB of LDS: still two workgroups per CU
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv_stem_f16x3_kernel(const ConvF16Args a) {
  constexpr int kStemMaxP = ((kStemTH - 1) * 2 + 7) * ((kStemTW - 1) * 2 + 7), NPL = (kStemMaxP + 511) / 512;
  constexpr int BN = 64, BK = 32, WN = BN / 2, FM = kStemTH / 4, FN = WN / 16;
  __shared__ __attribute__((aligned(16))) uint16_t sP[2][(kStemMaxP + 1) * 4];   // [hi, lo][pixel][4 ch]; + a zero pixel
  __shared__ __attribute__((aligned(16))) uint16_t sW[kStemMaxKt][2][BN * BK];
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int grp = blockIdx.z;
  const ConvGroupArgs g = pick_group(a, grp);
  const int tiles_x = (a.Wo + kStemTW - 1) / kStemTW, tiles_y = (a.Ho + kStemTH - 1) / kStemTH;
  const int img = blockIdx.x / (tiles_x * tiles_y), trem = blockIdx.x - img * (tiles_x * tiles_y);
  const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
  const int oy0 = ty * kStemTH, ox0 = tx * kStemTW;
  const int PW = (kStemTW - 1) * a.stride + a.kw, NP = ((kStemTH - 1) * a.stride + a.kh) * PW;
  const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
  const int nk = a.Kp / BK, taps = a.kh * a.kw;

  float sa = g.xscale;
  if (g.xmax) {
    const float mx = wave_max(g.xmax[lane * kShardStride]);
    sa = mx > 0.f ? pow2_scale(mx) : 1.0f;
  }
  const float inv = g.inv_w / sa;

  // the weights of every K-tile: one 16-row x 64-B piece per wave and K-tile (conv_f16x3_kernel's load_w, BN = 64)
  const u32x4 qWh = make_rsrc_words(g.wh, (int64_t)a.Cout * a.Kp * 2);
  const u32x4 qWl = make_rsrc_words(g.wl, (int64_t)a.Cout * a.Kp * 2);
  {
    const int wimg = wave / (BN / 16), rb = wave % (BN / 16);
    const int row = rb * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 2);
    const uint32_t vo = (uint32_t)((row * a.Kp + c * 8) * 2);
    for (int kt = 0; kt < nk; ++kt) {
      const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)(&sW[kt][wimg][rb * 16 * BK]));
      const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)(kt * BK * 2));
      if (wimg)
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWl), "s"(so), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWh), "s"(so), "{m0}"(dst) : "memory");
    }
  }
  // the input patch: pixel q = t + 512 k of the patch, one float4 (4 channels) each
  const rsrc_t rX = make_rsrc(g.x, (int64_t)a.N * a.H * a.W * 16);
  float4 pv[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int q = t + 512 * k, py = q / PW, px = q - py * PW;
    const int iy = iy0 + py, ix = ix0 + px;
    const bool ok = q < NP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    const uint32_t vo = ok ? (uint32_t)(((img * a.H + iy) * a.W + ix) * 16) : kBufOob;
    pv[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo, 0, 0));
  }
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int q = t + 512 * k;
    if (q < NP) {
      uint16_t h[4], l[4];
      split_h(pv[k].x * sa, h[0], l[0]);
      split_h(pv[k].y * sa, h[1], l[1]);
      split_h(pv[k].z * sa, h[2], l[2]);
      split_h(pv[k].w * sa, h[3], l[3]);
      *reinterpret_cast<uint2*>(&sP[0][q * 4]) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
      *reinterpret_cast<uint2*>(&sP[1][q * 4]) = make_uint2(l[0] | (uint32_t)l[1] << 16, l[2] | (uint32_t)l[3] << 16);
    }
  }
  if (t < 2) *reinterpret_cast<uint2*>(&sP[t][kStemMaxP * 4]) = make_uint2(0u, 0u);   // the zero taps' pixel
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragment row = local pixel wm * 16 FM + i * 16 + (lane & 15): tile row wm * FM + i, column lane & 15; K chunk
  // lane >> 4 = taps 8 kt + 2 (lane >> 4) + (0, 1), 4 channels each (conv_f16x3_kernel's STEM K order)
  const int c = lane >> 4, col = lane & 15;
  for (int kt = 0; kt < nk; ++kt) {
    bf16x8 ah[FM], al[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int r = wm * FM + i;
      uint2 hv[2], lv[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tap = kt * 8 + 2 * c + h, ky = tap / a.kw, kx = tap - ky * a.kw;
        const int pix = tap < taps ? (r * a.stride + ky) * PW + col * a.stride + kx : kStemMaxP;
        hv[h] = *reinterpret_cast<const uint2*>(&sP[0][pix * 4]);
        lv[h] = *reinterpret_cast<const uint2*>(&sP[1][pix * 4]);
      }
      ah[i] = __builtin_bit_cast(bf16x8, make_uint4(hv[0].x, hv[0].y, hv[1].x, hv[1].y));
      al[i] = __builtin_bit_cast(bf16x8, make_uint4(lv[0].x, lv[0].y, lv[1].x, lv[1].y));
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int row = wn * WN + j * 16 + (lane & 15);
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&sW[kt][0][cswz(row, c)]);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&sW[kt][1][cswz(row, c)]);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        acc[i][j] = mfma16<true>(bh, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bl, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bh, al[i], acc[i][j]);
      }
    }
  }

  const int lk = lane >> 4;
  float ymx = 0.f;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int oy = oy0 + wm * FM + i, ox = ox0 + col;
    if (oy >= a.Ho || ox >= a.Wo) continue;
    const int64_t mo = ((int64_t)img * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int no = wn * WN + j * 16 + 4 * lk;
      const f32x4 v = conv_tail(g, conv_lin(g, acc[i][j], inv, no), mo, no, a.Cout);
#pragma unroll
      for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
    }
  }
  __syncthreads();   // the patch is free for the max fold
  if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.z * 13, reinterpret_cast<float*>(&sP[0][0]));
}

// The stem with ResNet's max-pool (3 x 3 / stride 2 / pad 1, dimpnet.py's backbone conv1 -> bn1 -> relu -> maxpool)
// fused in (MMT_CONV_POOL): a workgroup owns an 8 x 8 tile of POOLED outputs, computes the 17 x 17 stem outputs
// their windows read (rows 16 ty - 1 .. 16 ty + 15; the shared edge row / column is computed by both neighbours), max-
// pools them from the LDS and writes only the pooled map -- the full-resolution stem map (4x the pooled bytes) is never
// written or read back, and the separate max-pool launch goes.  The 289 stem pixels run as 19 MFMA row fragments
// (five per wave row, the twentieth idle) over the conv_stem_f16x3_kernel K order; same products, same order, and the
// window max in maxpool4_kernel's order over the valid pixels (-inf elsewhere): the pooled map is the two kernels'
// bit for bit.  7 x 7 / stride 2 / 4 channels / 64 outputs only: K = 49 taps x 4 = 196, so the last of the seven
// 32-deep K-tiles holds one tap and only its first 16-B chunk of each weight row is staged (the other three lanes'
// fragments read the same finite weights against the zero pixel).
constexpr int kPoolS = 2 * kPoolT + 1, kPoolPx = kPoolS * kPoolS;                // 8 x 8 pooled, 17 x 17 stem
constexpr int kPoolPW = (kPoolS - 1) * 2 + 7, kPoolMaxP = kPoolPW * kPoolPW;      // 39 x 39 input pixels
constexpr int kPoolHalf = (kPoolPW + 1) / 2;                                         // a row's even columns
constexpr int kPoolLdsP = 2 * (kPoolMaxP + 1) * 4 * 2;                               // patch hi / lo (+ zero pixel)
constexpr int kPoolLdsW = 6 * 2 * 64 * 32 * 2 + 2 * 64 * 8 * 2;                     // K-tiles 0-5, chunk 0 of 6
constexpr int kPoolLds = kPoolLdsP + kPoolLdsW > kPoolPx * 64 * 4 ? kPoolLdsP + kPoolLdsW : kPoolPx * 64 * 4;
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv_stem_pool_f16x3_kernel(
    const ConvF16Args a, int PHo, int PWo) {
  constexpr int BN = 64, BK = 32, WN = BN / 2, FM = 5, FN = WN / 16, NPL = (kPoolMaxP + 511) / 512;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kPoolLds];
  uint16_t* sPh = reinterpret_cast<uint16_t*>(lds);
  uint16_t* sPl = sPh + (kPoolMaxP + 1) * 4;
  uint16_t* sW = reinterpret_cast<uint16_t*>(lds + kPoolLdsP);          // [6][2][64 x 32], cswz rows
  uint16_t* sW6 = sW + 6 * 2 * BN * BK;                                  // [2][64][8]: K-tile 6, chunk 0
  float* sOut = reinterpret_cast<float*>(lds);                           // [289][64] after the K loop
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const ConvGroupArgs g = pick_group(a, blockIdx.z);
  const int tiles_x = (PWo + kPoolT - 1) / kPoolT, tiles_y = (PHo + kPoolT - 1) / kPoolT;
  const int img = blockIdx.x / (tiles_x * tiles_y), trem = blockIdx.x - img * (tiles_x * tiles_y);
  const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
  const int sy0 = 2 * kPoolT * ty - 1, sx0 = 2 * kPoolT * tx - 1;       // the stem tile's first output row / col
  const int iy0 = sy0 * 2 - a.pad, ix0 = sx0 * 2 - a.pad;

  float sa = g.xscale;
  if (g.xmax) {
    const float mx = wave_max(g.xmax[lane * kShardStride]);
    sa = mx > 0.f ? pow2_scale(mx) : 1.0f;
  }
  const float inv = g.inv_w / sa;

  const u32x4 qWh = make_rsrc_words(g.wh, (int64_t)a.Cout * a.Kp * 2);
  const u32x4 qWl = make_rsrc_words(g.wl, (int64_t)a.Cout * a.Kp * 2);
  {
    const int wimg = wave / (BN / 16), rb = wave % (BN / 16);
    const int row = rb * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 2);
    const uint32_t vo = (uint32_t)((row * a.Kp + c * 8) * 2);
    for (int kt = 0; kt < 6; ++kt) {
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(lptr_t)(&sW[(kt * 2 + wimg) * BN * BK + rb * 16 * BK]));
      const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)(kt * BK * 2));
      if (wimg)
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWl), "s"(so), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWh), "s"(so), "{m0}"(dst) : "memory");
    }
    if (wave < 2) {   // K-tile 6, chunk 0 (K 192-199) of row = lane: 16 B per lane, rows contiguous
      const uint32_t dst = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lptr_t)(&sW6[wave * BN * 8]));
      const uint32_t vo6 = (uint32_t)((lane * a.Kp + 6 * BK) * 2);
      if (wave)
        asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(vo6), "s"(qWl), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(vo6), "s"(qWh), "{m0}"(dst) : "memory");
    }
  }
  const rsrc_t rX = make_rsrc(g.x, (int64_t)a.N * a.H * a.W * 16);
  float4 pv[NPL];
  int lq[NPL];   // the pixel's LDS slot: each patch row stores its even columns, then its odd ones (see below)
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int q = t + 512 * k, py = q / kPoolPW, px = q - py * kPoolPW;
    lq[k] = py * kPoolPW + (px & 1) * kPoolHalf + (px >> 1);
    const int iy = iy0 + py, ix = ix0 + px;
    const bool ok = q < kPoolMaxP && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    const uint32_t vo = ok ? (uint32_t)(((img * a.H + iy) * a.W + ix) * 16) : kBufOob;
    pv[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo, 0, 0));
  }
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int q = t + 512 * k;
    if (q < kPoolMaxP) {
      uint16_t h[4], l[4];
      split_h(pv[k].x * sa, h[0], l[0]);
      split_h(pv[k].y * sa, h[1], l[1]);
      split_h(pv[k].z * sa, h[2], l[2]);
      split_h(pv[k].w * sa, h[3], l[3]);
      *reinterpret_cast<uint2*>(&sPh[lq[k] * 4]) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
      *reinterpret_cast<uint2*>(&sPl[lq[k] * 4]) = make_uint2(l[0] | (uint32_t)l[1] << 16, l[2] | (uint32_t)l[3] << 16);
    }
  }
  if (t < 2) *reinterpret_cast<uint2*>(&(t ? sPl : sPh)[kPoolMaxP * 4]) = make_uint2(0u, 0u);   // the zero pixel
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // fragment i of wave row wm: stem pixels p = (wm + 4 i) * 16 + (lane & 15) of the 17 x 17 tile (p >= 289: idle).
  // The stride-2 stem reads input columns 2 sc + kx: with each patch row stored as its even columns then its odd ones,
  // the 16 lanes of a fragment column read 16 consecutive 8-B slots (32 banks) for any tap, and the next lane group's
  // tap (kx + 2, same parity) the slots one further -- the same addresses but for its last lane, whose banks are free.
  // Interleaved, the slots were 16 B apart and that last lane met lane 0's banks: 38 % of the kernel's LDS cycles
  // were bank conflicts (r05_pmc_mfma_dimp_b1.txt)
  const int c = lane >> 4, col = lane & 15;
  int pbase[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int p = (wm + 4 * i) * 16 + col, sr = p / kPoolS, sc = p - sr * kPoolS;
    pbase[i] = p < kPoolPx ? (sr * 2) * kPoolPW + sc : -1;
  }
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool last_idle = wm == 3;   // fragment 19 (wave row 3, i = 4) holds no pixel
#pragma unroll
  for (int kt = 0; kt < 7; ++kt) {
    bf16x8 ah[FM], al[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      uint2 hv[2], lv[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int tap = kt * 8 + 2 * c + h, ky = tap / 7, kx = tap - ky * 7;
        const int pix = tap < 49 && pbase[i] >= 0 ? pbase[i] + ky * kPoolPW + (kx & 1) * kPoolHalf + (kx >> 1)
                                                  : kPoolMaxP;
        hv[h] = *reinterpret_cast<const uint2*>(&sPh[pix * 4]);
        lv[h] = *reinterpret_cast<const uint2*>(&sPl[pix * 4]);
      }
      ah[i] = __builtin_bit_cast(bf16x8, make_uint4(hv[0].x, hv[0].y, hv[1].x, hv[1].y));
      al[i] = __builtin_bit_cast(bf16x8, make_uint4(lv[0].x, lv[0].y, lv[1].x, lv[1].y));
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int row = wn * WN + j * 16 + (lane & 15);
      bf16x8 bh, bl;
      if (kt < 6) {
        bh = *reinterpret_cast<const bf16x8*>(&sW[(kt * 2 + 0) * BN * BK + cswz(row, c)]);
        bl = *reinterpret_cast<const bf16x8*>(&sW[(kt * 2 + 1) * BN * BK + cswz(row, c)]);
      } else {
        bh = *reinterpret_cast<const bf16x8*>(&sW6[row * 8]);
        bl = *reinterpret_cast<const bf16x8*>(&sW6[BN * 8 + row * 8]);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if (i == FM - 1 && last_idle) continue;
        acc[i][j] = mfma16<true>(bh, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bl, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bh, al[i], acc[i][j]);
      }
    }
  }
  __syncthreads();   // the patch and weights are free: the stem tile goes to sOut

  // bias + ReLU per stem pixel (-inf outside the stem map: the pool's padding); 16-B chunk q of pixel p at
  // q ^ (p & 15) (the 16 lanes of one fragment column write 16 distinct chunks: no bank conflict)
  const int lk = lane >> 4;
  float ymx = 0.f;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int p = (wm + 4 * i) * 16 + col;
    if (p >= kPoolPx) continue;
    const int sr = p / kPoolS, sc = p - sr * kPoolS, oy = sy0 + sr, ox = sx0 + sc;
    const bool valid = oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int no = wn * WN + j * 16 + 4 * lk;
      f32x4 v = conv_lin(g, acc[i][j], inv, no);   // (the stem kernel's arithmetic: bit-identical to stem + pool)
      if (g.flags & MMT_CONV_RELU)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
      if (valid) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
      } else {
        v = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
      *reinterpret_cast<f32x4*>(&sOut[p * 64 + (((no >> 2) ^ (p & 15)) << 2)]) = v;
    }
  }
  __syncthreads();
  // the pooled 8 x 8 tile: thread t takes 4 channels (chunk t & 15) of pooled pixels t >> 4 and (t >> 4) + 32
  {
    const int q = t & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pq = (t >> 4) + 32 * h, pr = pq >> 3, pc = pq & 7;
      const int py = kPoolT * ty + pr, px = kPoolT * tx + pc;
      if (py >= PHo || px >= PWo) continue;
      f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int p = (2 * pr + dy) * kPoolS + 2 * pc + dx;
          const f32x4 v = *reinterpret_cast<const f32x4*>(&sOut[p * 64 + ((q ^ (p & 15)) << 2)]);
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
        }
      *reinterpret_cast<float4*>(g.y + (((int64_t)img * PHo + py) * PWo + px) * 64 + 4 * q) =
          make_float4(m[0], m[1], m[2], m[3]);
    }
  }
  __syncthreads();   // sOut is free for the max fold
  if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.z * 13, reinterpret_cast<float*>(lds));
}

// The generic conv with a deeper operand pipeline.  conv_f16x3_kernel keeps one K-tile of weights and two of
// activations in flight per workgroup (about 48 KB), which, at the several-microsecond latency of a loaded memory
// system, caps a workgroup near 20 GB/s and the K loop at about 1.5 us per 32-deep K-tile -- measured: removing two
// of the three MFMAs and the whole activation split / stash together saves only a third of the kernel's time.  Here
// the activation loads are inline-asm buffer loads (the compiler neither counts nor waits for them; every wait is
// written out, naming the registers it guards), so the weights can go two K-tiles ahead into the three-stage ring and
// the activations NR = 3 K-tiles ahead into three register sets without the compiler draining one queue to reach the
// other.  Step j waits for A(j + 1) -- NW + NA younger operations -- BEFORE K-tile j is multiplied, issues W(j + 2)
// then A(j + 3), and splits and stashes A(j + 1) in the same scheduling region as K-tile j's MFMAs (no inline asm
// between them), so the split's VALU work and the LDS stores issue between the MFMAs instead of after them while every
// wave of the CU sits in the same phase between two barriers; then it waits for W(j + 1) and passes the barrier.
// Same products, same summation order as conv_f16x3_kernel (bit-identical).
template <int BN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv_f16x3_deep_kernel(const ConvF16Args a) {
  constexpr int BM = 128, BK = 32, NWS = 3, NR = 3;
  constexpr int WN = BN / 2, FM = BM / 64, FN = WN / 16;
  constexpr int NW = BN / 64;                  // W LDS-DMA pieces per wave per K-tile
  constexpr int NA = 2;                        // A loads per thread per K-tile
  constexpr int WAIT_A = (NR - 1) * (NW + NA); // younger operations when the prologue waits for A(0)
  constexpr int WAIT_W = 2 * NA + NW;          // ... when W(j + 1) is waited for (A(j + 2), W(j + 2), A(j + 3))
  constexpr int WAIT_AE = (NR - 2) * (NW + NA); // ... when A(j + 1) is, before step j's loads
  // one LDS array (the operand rings, then the epilogue's staged tile: 128 x BN floats <= its size)
  __shared__ __attribute__((aligned(16))) uint16_t smem_dk[2 * 2 * BM * BK + NWS * 2 * BN * BK];
  auto& sA = *reinterpret_cast<uint16_t(*)[2][2][BM * BK]>(smem_dk);
  auto& sW = *reinterpret_cast<uint16_t(*)[NWS][2][BN * BK]>(smem_dk + 2 * 2 * BM * BK);
  static_assert(128 * BN * 4 <= (int)sizeof(smem_dk), "staged epilogue tile");
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int grp = blockIdx.z / a.ks, slice = blockIdx.z - grp * a.ks;
  const ConvGroupArgs g = pick_group(a, grp);
  const int M = a.N * a.Ho * a.Wo;
  // XCD-aware tile order (grid.x = M tiles x N tiles): the workgroups of XCD x (= b % 8) take a contiguous range of
  // tile ids, N fastest, so the column-tile siblings of an activation tile run on one XCD and share its L2 (the
  // activation tile is fetched from beyond the L2 once per XCD instead of once per column tile)
  // (the default: mfDiMP 6 350 -> 6 394 frames/s in two rounds; applied only to wide outputs and short launches it
  // measured level, although layer1 conv3 alone, without its residual, runs 128 -> 150 us in this order; against
  // M tiles fastest over the whole chip, profiles/r04_ab_conv_xcd_order.txt)
  int m0, n0;
  {
    const int gn = a.Cout / BN, ntl = gridDim.x, b = blockIdx.x;
    if (a.xcd_order) {
      const int x = b & 7, j = b >> 3, q = ntl >> 3, r8 = ntl & 7;
      const int id = (x < r8 ? x * (q + 1) : r8 * (q + 1) + (x - r8) * q) + j;
      m0 = (id / gn) * BM;
      n0 = (id - (id / gn) * gn) * BN;
    } else {
      const int gm = ntl / gn;
      m0 = (b % gm) * BM;
      n0 = (b / gm) * BN;
    }
  }

  float sa = g.xscale;
  if (g.xmax) {
    const float mx = wave_max(g.xmax[lane * kShardStride]);
    sa = mx > 0.f ? pow2_scale(mx) : 1.0f;
  }
  // fused downsample: both sources split at the smaller scale, so one accumulator holds both sums
  const bool ds = a.Cin2 > 0;
  if (ds) {
    float sb = g.x2scale;
    if (g.x2max) {
      const float mx = wave_max(g.x2max[lane * kShardStride]);
      sb = mx > 0.f ? pow2_scale(mx) : 1.0f;
    }
    sa = fminf(sa, sb);
  }
  const float inv = g.inv_w / sa;

  const int ac = t & 3;   // A load slot: row (pixel) t >> 2, K chunk ac (8 values)
  // (the slot's geometry stays the one-trip loop over one-element arrays it was measured as: the compiler promotes
  // them only once the loop is unrolled, and written as scalars it allocates the whole kernel's registers differently)
  bool mval[1];
  int iy0[1], ix0[1];
  uint32_t xrow[1], xrow2[1];
#pragma unroll
  for (int sl = 0; sl < 1; ++sl) {
    const int m = m0 + (t >> 2);
    mval[sl] = m < M;
    iy0[sl] = ix0[sl] = 0;
    xrow[sl] = xrow2[sl] = 0;
    if (mval[sl]) {
      const int nimg = m / (a.Ho * a.Wo);
      const int r = m - nimg * a.Ho * a.Wo;
      const int oy = r / a.Wo, ox = r - oy * a.Wo;
      iy0[sl] = oy * a.stride - a.pad;
      ix0[sl] = ox * a.stride - a.pad;
      xrow[sl] = (uint32_t)(nimg * a.H * a.W * a.Cin);
      // the downsample's input pixel (1 x 1, no padding): its float offset, channel 0
      if (ds) xrow2[sl] = (uint32_t)(((nimg * a.H2 + oy * a.stride2) * a.W2 + ox * a.stride2) * a.Cin2);
    }
  }
  const u32x4 qX = make_rsrc_words(g.x, (int64_t)a.N * a.H * a.W * a.Cin * 4);
  const u32x4 qX2 = make_rsrc_words(ds ? g.x2 : g.x, ds ? (int64_t)a.N * a.H2 * a.W2 * a.Cin2 * 4 : 0);
  const int nk1 = ds ? a.Cin / BK : 1 << 30;   // K-tiles of the first source (1 x 1 conv3: its Cin)
  const int nk = a.Kp / BK;
  const int kt0 = (int)((int64_t)slice * nk / a.ks), nt = (int)((int64_t)(slice + 1) * nk / a.ks) - kt0;
  const int cpt = a.Cin / BK;

  struct DeepRegs {   // native vectors: an inline-asm register operand, not a struct in memory
    f32x4 a[2];
  };
  DeepRegs r[NR];
  // K-tile i of the slice (zeros past it: an out-of-range offset, no traffic) into register set `set`.  The calls
  // come in order i = 0, 1, 2, ...: the (tap, chunk) position advances by one chunk per call (wave-uniform
  // counters instead of two integer divisions per K-tile)
  int a_ch, a_ky, a_kx;
  {
    const int tap = kt0 / cpt;
    a_ch = kt0 - tap * cpt;
    a_ky = tap / a.kw;
    a_kx = tap - a_ky * a.kw;
  }
  auto load_a = [&](int i, DeepRegs& set) {
    const int c0 = a_ch * BK + ac * 8, ky = a_ky, kx = a_kx;
    if (++a_ch == cpt) {
      a_ch = 0;
      if (++a_kx == a.kw) {
        a_kx = 0;
        ++a_ky;
      }
    }
    // the fused downsample's K-tiles (wave-uniform; selects, not a branch, so the loads stay straight-line code for
    // tools/isa_audit.py): x2 at the output pixel's stride2 position
    const bool second = kt0 + i >= nk1;
    const int c2 = (kt0 + i - nk1) * BK + ac * 8;
    const u32x4 qA = second ? qX2 : qX;
    const int iy = iy0[0] + ky, ix = ix0[0] + kx;
    // (bitwise, not short-circuit: no control flow around the loads)
    const bool inb = (iy >= 0) & (iy < a.H) & (ix >= 0) & (ix < a.W);
    const bool ok = (i < nt) & mval[0] & (second | inb);
    const uint32_t off1 = xrow[0] + (uint32_t)((iy * a.W + ix) * a.Cin + c0), off2 = xrow2[0] + (uint32_t)c2;
    const uint32_t vo = ok ? (second ? off2 : off1) * 4 : kBufOob;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(set.a[0]) : "v"(vo), "s"(qA) : "memory");
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen offset:16" : "=v"(set.a[1]) : "v"(vo), "s"(qA) : "memory");
  };
  const u32x4 qWh = make_rsrc_words(g.wh, (int64_t)a.Cout * a.Kp * 2);
  const u32x4 qWl = make_rsrc_words(g.wl, (int64_t)a.Cout * a.Kp * 2);
  auto load_w = [&](int i, int st) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int p = wave * NW + j, img = p / (BN / 16), rb = p % (BN / 16);
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(lptr_t)(&sW[st][img][rb * 16 * BK]));
      const int row = rb * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 2);
      const uint32_t vo = i < nt ? (uint32_t)(((n0 + row) * a.Kp + c * 8) * 2) : kBufOob;
      const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)((kt0 + i) * BK * 2));
      if (img)
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWl), "s"(so), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWh), "s"(so), "{m0}"(dst) : "memory");
    }
  };
  // the register set's loads done: all but the CNT youngest vector-memory operations (the set named as read-write,
  // so nothing reads it above this point)
  auto wait_set = [&](DeepRegs& set, auto cnt) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(set.a[0]), "+v"(set.a[1]) : "n"(decltype(cnt)::value) : "memory");
  };
  auto keep_set = [&](DeepRegs& set) {   // the set's registers live up to here (no code, no wait)
    asm volatile("" : "+v"(set.a[0]), "+v"(set.a[1]));
  };
  auto pack2 = [&](float x, float y, uint32_t& h, uint32_t& l) {
    uint16_t hx, lx, hy, ly;
    split_h(x * sa, hx, lx);
    split_h(y * sa, hy, ly);
    h = hx | (uint32_t)hy << 16;
    l = lx | (uint32_t)ly << 16;
  };
  auto stash = [&](const DeepRegs& rr, int st) {   // the prologue's: K-tile 0, nothing to weave it into
    const f32x4 &x0 = rr.a[0], &x1 = rr.a[1];
    uint4 hv, lv;
    pack2(x0[0], x0[1], hv.x, lv.x);
    pack2(x0[2], x0[3], hv.y, lv.y);
    pack2(x1[0], x1[1], hv.z, lv.z);
    pack2(x1[2], x1[3], hv.w, lv.w);
    const int ar = t >> 2;
    *reinterpret_cast<uint4*>(&sA[st][0][cswz(ar, ac)]) = hv;
    *reinterpret_cast<uint4*>(&sA[st][1][cswz(ar, ac)]) = lv;
  };
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // K-tile (sta, stw) multiplied with the next K-tile's split woven in: all fragment reads first, then after
  // every MFMA triple (BN 128: every other) one pack2 (two values) of the split -- fenced (sched_barrier) so the
  // compiler keeps the weave instead of clustering the MFMAs -- and the stash's LDS stores last
  auto compute_split = [&](int sta, int stw, const DeepRegs& rr, int st) {
    const int c = lane >> 4;
    bf16x8 ah[FM], al[FM], bh[FN], bl[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int row = wm * (BM / 4) + i * 16 + (lane & 15);
      ah[i] = *reinterpret_cast<const bf16x8*>(&sA[sta][0][cswz(row, c)]);
      al[i] = *reinterpret_cast<const bf16x8*>(&sA[sta][1][cswz(row, c)]);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int row = wn * WN + j * 16 + (lane & 15);
      bh[j] = *reinterpret_cast<const bf16x8*>(&sW[stw][0][cswz(row, c)]);
      bl[j] = *reinterpret_cast<const bf16x8*>(&sW[stw][1][cswz(row, c)]);
    }
    uint32_t hw[4], lw[4];
    constexpr int NP = 4, NT = FM * FN, EVERY = NT / NP;
    static_assert(NT == NP * EVERY, "every pack2 has its MFMA triple");
    int p = 0;
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        // empty asm on the operands pins the order (instruction selection moves pure operations across fences)
        asm volatile("" : "+v"(acc[i][j]));
        acc[i][j] = mfma16<true>(bh[j], ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bl[j], ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bh[j], al[i], acc[i][j]);
        asm volatile("" : "+v"(acc[i][j]));
        __builtin_amdgcn_sched_barrier(0);
        if ((j * FM + i) % EVERY == EVERY - 1) {
          const f32x4& x = rr.a[p >> 1];
          float x0 = x[(p & 1) * 2], x1 = x[(p & 1) * 2 + 1];
          asm volatile("" : "+v"(x0), "+v"(x1));
          pack2(x0, x1, hw[p], lw[p]);
          asm volatile("" : "+v"(hw[p]), "+v"(lw[p]));
          ++p;
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    const int ar = t >> 2;
    *reinterpret_cast<uint4*>(&sA[st][0][cswz(ar, ac)]) = make_uint4(hw[0], hw[1], hw[2], hw[3]);
    *reinterpret_cast<uint4*>(&sA[st][1][cswz(ar, ac)]) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
  };

  // prologue: the loads of steps -NR .. -1 (W(j + 2) where j + 2 >= 0, A(j + NR)), so the steady-state counts hold
  // from step 0 on
#pragma unroll
  for (int j = -NR; j < 0; ++j) {
    if (j + 2 >= 0) load_w(j + 2, j + 2);
    load_a(j + NR, r[j + NR]);
  }
  wait_set(r[0], std::integral_constant<int, WAIT_A>{});
  stash(r[0], 0);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_W) : "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  for (int i0 = 0; i0 < nt; i0 += 6) {
#pragma unroll
    for (int u = 0; u < 6; ++u) {
      const int j = i0 + u;
      if (j >= nt) break;
      wait_set(r[(u + 1) % NR], std::integral_constant<int, WAIT_AE>{});
      load_w(j + 2, (u + 2) % 3);
      load_a(j + NR, r[u % NR]);
      compute_split(u & 1, u % 3, r[(u + 1) % NR], (u + 1) & 1);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_W) : "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
  // the zero-loads past the slice land before the LDS is left -- and before their registers are reused: the last
  // sets' loads are dead to the compiler, which would otherwise hand their registers to the epilogue while the
  // loads are still in flight (the landing zeros then overwrite epilogue values), so every set is named live across
  // the wait
  wait_set(r[0], std::integral_constant<int, 0>{});
#pragma unroll
  for (int k = 1; k < NR; ++k) keep_set(r[k]);

  const int li = lane & 15, lk = lane >> 4;
  if (a.ks > 1) {
    const int G = gridDim.z / a.ks;
    float* pb = a.part + ((int64_t)slice * G + grp) * M * a.Cout;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mo = m0 + wm * (BM / 4) + i * 16 + li;
      if (mo >= M) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int no = n0 + wn * WN + j * 16 + 4 * lk;
        const f32x4 v = acc[i][j] * inv;
        *reinterpret_cast<float4*>(pb + (int64_t)mo * a.Cout + no) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    return;
  }
  float ymx;
  if (a.staged_epi && (int64_t)M * a.Cout * 4 < ((int64_t)1 << 31)) {
    ymx = conv_store_tile_staged<FN, BN>(g, acc, inv, reinterpret_cast<float*>(smem_dk), wm, wn, lane, m0, M, n0,
                                         a.Cout, M);
    if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.y * 7 + blockIdx.z * 13, reinterpret_cast<float*>(smem_dk));
    return;
  }
  int64_t mo[FM];
  bool mv[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    mo[i] = m0 + wm * (BM / 4) + i * 16 + li;
    mv[i] = mo[i] < M;
  }
  ymx = conv_store_tile<FM, FN>(g, acc, inv, mo, mv, n0 + wn * WN + 4 * lk, a.Cout, M);
  if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.y * 7 + blockIdx.z * 13, reinterpret_cast<float*>(&sA[0][0][0]));
}

// 3 x 3 / stride 1 / pad 1 convolutions with the input PATCH staged once per 32-channel chunk.  The generic kernel
// above gathers, splits and stashes a K-tile of activations for every (tap, chunk) K-tile, so each input element is
// loaded, split into fp16 hi / lo and written to the LDS nine times.  Here a workgroup's tile is 128 consecutive output
// pixels of one image (raster order) and, per chunk of 32 input channels, the rows of the input those pixels' nine taps
// read -- (rows + 2) x (W + 2) pixels, zeros outside the image -- are loaded and split ONCE into an LDS patch; the nine
// taps then read their A fragments from it at pixel offsets (dy, dx), and only the weights (one 32-deep K-tile per tap,
// LDS-DMA into a two-stage ring) move per tap.  Patch layout: pixel P = 64 B per half (32 channels), 16-B chunk q of
// P at q ^ (((P >> 2) & 1) << 1): the fragment reads (16 consecutive pixels x 4 chunks per ds_read_b128 lane group)
// are bank-conflict-free for any start pixel (exhaustive check over start offsets; a tile row that wraps to the next
// image row costs at most one 2-way conflict).  K order: chunk-major, tap-minor (the weights' K-tile tap * Cin / 32 +
// chunk); split-K slices take ranges of chunks.  Same products as conv_f16x3_kernel, summed in a different fp32 order.
constexpr int kPatchNPL = kPatchMaxPx * 8 / 512;   // float4 loads per thread (kPatchMaxPx pixels x 32 channels)
template <int BN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void conv3x3_patch_f16x3_kernel(
    const ConvF16Args a, int tiles_per_img, int patch_px) {
  constexpr int BM = 128, BK = 32;
  constexpr int WN = BN / 2, FM = 2, FN = WN / 16, NW = BN / 64;
  extern __shared__ __attribute__((aligned(16))) uint16_t dynlds[];
  // fixed offsets (immediate fields of the LDS instructions), sized for the largest patch
  uint16_t* const sPh = dynlds;                          // [kPatchMaxPx][32] hi
  uint16_t* const sPl = dynlds + kPatchMaxPx * 32;       // lo
  uint16_t* const sWb = dynlds + 2 * kPatchMaxPx * 32;   // [2 stages][hi, lo][BN * BK]
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int grp = blockIdx.z / a.ks, slice = blockIdx.z - grp * a.ks;
  const ConvGroupArgs g = pick_group(a, grp);
  const int HW = a.Ho * a.Wo, Wd = a.W, PW = a.W + 2;
  // the tile: global output pixels [g0, gend) -- per image (tiles_per_img > 0: 128 raster pixels of one image) or
  // over the flattened batch (tiles_per_img == 0: no partial tile at each image's end; a tile then spans at most two
  // images, HW >= 128): segment A = image nA's output rows yA0.. (patch rows 0 .. rowsA - 1 with their halo rows),
  // segment B = the next image's first rows (patch rows rowsA .., its own halo above and below)
  int g0, gend, nA, yA0, rowsA, rowsB = 0;
  if (tiles_per_img > 0) {
    const int img = blockIdx.x / tiles_per_img, o0 = (blockIdx.x - img * tiles_per_img) * BM;
    g0 = img * HW + o0;
    gend = img * HW + min(o0 + BM, HW);
  } else {
    g0 = blockIdx.x * BM;
    gend = min(g0 + BM, a.N * HW);
  }
  nA = g0 / HW;
  yA0 = (g0 - nA * HW) / Wd;
  rowsA = (min(gend, (nA + 1) * HW) - nA * HW - 1) / Wd - yA0 + 3;
  if (gend > (nA + 1) * HW) rowsB = (gend - (nA + 1) * HW - 1) / Wd + 3;
  const int npx = (rowsA + rowsB) * PW;   // patch pixels of this tile
  const int n0 = blockIdx.y * BN;

  float sa = g.xscale;
  if (g.xmax) {
    const float mx = wave_max(g.xmax[lane * kShardStride]);
    sa = mx > 0.f ? pow2_scale(mx) : 1.0f;
  }
  const float inv = g.inv_w / sa;

  const int nc = a.Cin / BK;                              // 32-channel chunks
  const int c0 = (int)((int64_t)slice * nc / a.ks), c1 = (int)((int64_t)(slice + 1) * nc / a.ks);

  // the patch: float4 f = t + 512 j is channels 4 (f & 7) .. + 3 of patch pixel f >> 3
  const rsrc_t rX = make_rsrc(g.x, (int64_t)a.N * a.H * a.W * a.Cin * 4);
  float4 pv[kPatchNPL];
  auto load_patch = [&](int c) {
#pragma unroll
    for (int j = 0; j < kPatchNPL; ++j) {
      const int f = t + 512 * j, px = f >> 3, part = f & 7;
      const int pr = px / PW, pc = px - pr * PW;
      const bool segb = pr >= rowsA;
      const int im = segb ? nA + 1 : nA, iy = segb ? pr - rowsA - 1 : yA0 - 1 + pr, ix = pc - 1;
      const bool ok = px < npx && iy >= 0 && iy < a.H && ix >= 0 && ix < Wd;
      const uint32_t vo = ok ? (uint32_t)((((im * a.H + iy) * Wd + ix) * a.Cin + c * BK + 4 * part) * 4) : kBufOob;
      pv[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rX, vo, 0, 0));
    }
  };
  auto stash_patch = [&]() {
    // the thread id made opaque here, so the stash addresses are formed at each stash rather than hoisted out of
    // the chunk loop (they would take 12 VGPRs across it, and spill)
    int tt = t;
    asm volatile("" : "+v"(tt));
#pragma unroll
    for (int j = 0; j < kPatchNPL; ++j) {
      const int f = tt + 512 * j, px = f >> 3, part = f & 7;
      if (px < npx) {
        uint16_t h[4], l[4];
        split_h(pv[j].x * sa, h[0], l[0]);
        split_h(pv[j].y * sa, h[1], l[1]);
        split_h(pv[j].z * sa, h[2], l[2]);
        split_h(pv[j].w * sa, h[3], l[3]);
        const int off = px * 32 + (((part >> 1) ^ (((px >> 2) & 1) << 1)) << 3) + ((part & 1) << 2);
        *reinterpret_cast<uint2*>(sPh + off) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
        *reinterpret_cast<uint2*>(sPl + off) = make_uint2(l[0] | (uint32_t)l[1] << 16, l[2] | (uint32_t)l[3] << 16);
      }
    }
  };
  // weights: conv_f16x3_kernel's LDS-DMA pieces, K-tile (tap, chunk) = tap * nc + chunk
  const u32x4 qWh = make_rsrc_words(g.wh, (int64_t)a.Cout * a.Kp * 2);
  const u32x4 qWl = make_rsrc_words(g.wl, (int64_t)a.Cout * a.Kp * 2);
  auto load_w = [&](int kt, bool kv, int st) {
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int p = wave * NW + j, im = p / (BN / 16), rb = p % (BN / 16);
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          (uint32_t)(uintptr_t)(lptr_t)(sWb + (st * 2 + im) * BN * BK + rb * 16 * BK));
      const int row = rb * 16 + (lane >> 2), c = (lane & 3) ^ ((row >> 2) & 2);
      const uint32_t vo = kv ? (uint32_t)(((n0 + row) * a.Kp + c * 8) * 2) : kBufOob;
      const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)(kt * BK * 2));
      if (im)
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWl), "s"(so), "{m0}"(dst) : "memory");
      else
        asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(qWh), "s"(so), "{m0}"(dst) : "memory");
    }
  };

  // this lane's fragment rows: patch pixel of tap (0, 0) for output pixel g0 + 32 wm + 16 i + (lane & 15) (rows past
  // the tile's end read the tile's last pixel; their outputs are dropped)
  int pbase[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int o = min(g0 + wm * 32 + i * 16 + (lane & 15), gend - 1);
    const int n = o / HW, r = o - n * HW, y = r / Wd, x = r - y * Wd;
    pbase[i] = (n == nA ? y - yA0 : rowsA + y) * PW + x;
  }
  const int q = lane >> 4;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int tap, int st) {
    const int dy = tap / 3, dx = tap - dy * 3;
    bf16x8 ah[FM], al[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int P = pbase[i] + dy * PW + dx;
      const int off = P * 32 + ((q ^ (((P >> 2) & 1) << 1)) << 3);
      ah[i] = *reinterpret_cast<const bf16x8*>(sPh + off);
      al[i] = *reinterpret_cast<const bf16x8*>(sPl + off);
    }
    const uint16_t* wh = sWb + (st * 2) * BN * BK;
    const uint16_t* wl = sWb + (st * 2 + 1) * BN * BK;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int row = wn * WN + j * 16 + (lane & 15);
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(wh + cswz(row, q));
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(wl + cswz(row, q));
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        acc[i][j] = mfma16<true>(bh, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bl, ah[i], acc[i][j]);
        acc[i][j] = mfma16<true>(bh, al[i], acc[i][j]);
      }
    }
  };

  // prologue: the first chunk's patch and tap-0 weights
  load_patch(c0);
  load_w(c0, true, 0);
  stash_patch();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  int st = 0;
  for (int c = c0; c < c1; ++c) {
    const bool more = c + 1 < c1;
    // tap 0 (its weights and patch were waited for at the chunk boundary): the next tap's weights, then the next
    // chunk's patch behind them
    load_w(nc + c, true, st ^ 1);
    if (more) load_patch(c + 1);
    compute(0, st);
    st ^= 1;
    for (int tap = 1; tap < 9; ++tap) {
      // tap's weights landed (issued one tap ago; at tap 1 the next chunk's patch loads, issued after them, may stay
      // in flight) and every wave is past the previous tap, whose stage takes the next weights
      if (tap == 1 && more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPatchNPL) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // the next tap's weights, or the next chunk's tap 0 (zeros past the slice: nobody reads them)
      load_w(tap < 8 ? (tap + 1) * nc + c : c + 1, tap < 8 || more, st ^ 1);
      compute(tap, st);
      st ^= 1;
    }
    if (more) {
      // every wave is past its last read of this chunk's patch before it is overwritten
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      stash_patch();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const int li = lane & 15, lk = lane >> 4;
  if (a.ks > 1) {
    const int G = gridDim.z / a.ks;
    const int M = a.N * HW;
    float* pb = a.part + ((int64_t)slice * G + grp) * M * a.Cout;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int64_t mo = g0 + wm * 32 + i * 16 + li;
      if (mo >= gend) continue;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int no = n0 + wn * WN + j * 16 + 4 * lk;
        const f32x4 v = acc[i][j] * inv;
        *reinterpret_cast<float4*>(pb + mo * a.Cout + no) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    return;
  }
  // (fragment-shaped stores: the LDS-staged epilogue of the deep kernel pushed this kernel past 128 VGPRs into
  // scratch; the 3 x 3 layers are MFMA-bound, not store-bound)
  int64_t mo[FM];
  bool mv[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    mo[i] = g0 + wm * 32 + i * 16 + li;
    mv[i] = mo[i] < gend;
  }
  const float ymx = conv_store_tile<FM, FN>(g, acc, inv, mo, mv, n0 + wn * WN + 4 * lk, a.Cout, (int64_t)a.N * HW);
  __syncthreads();   // the LDS is free for the max fold
  if (g.ymax) fold_max<8>(g.ymax, ymx, blockIdx.x + blockIdx.y * 7 + blockIdx.z * 13, reinterpret_cast<float*>(dynlds));
}

// split-K: y = sum over the ks slices (in slice order) + bias (+ residual), ReLU, merge; grid (blocks, G), 4 channels
// per thread
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvF16Args a) {
  const int grp = blockIdx.y, G = gridDim.y;
  const ConvGroupArgs g = pick_group(a, grp);
  const int64_t M = (int64_t)a.N * a.Ho * a.Wo, q = M * a.Cout / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float ymx = 0.f;
  if (i < q) {
    const int64_t mo = i * 4 / a.Cout;
    const int no = (int)(i * 4 - mo * a.Cout);
    float4 p[kMaxSplitK];
#pragma unroll
    for (int s = 0; s < kMaxSplitK; ++s)
      if (s < a.ks) p[s] = reinterpret_cast<const float4*>(a.part + ((int64_t)s * G + grp) * M * a.Cout)[i];
    f32x4 v{p[0].x, p[0].y, p[0].z, p[0].w};
#pragma unroll
    for (int s = 1; s < kMaxSplitK; ++s)
      if (s < a.ks) v += f32x4{p[s].x, p[s].y, p[s].z, p[s].w};
    v = conv_out(g, v, mo, no, a.Cout);
#pragma unroll
    for (int e = 0; e < 4; ++e) ymx = fmaxf(ymx, fabsf(v[e]));
  }
  __shared__ float wmax[4];
  if (g.ymax) fold_max<4>(g.ymax, ymx, blockIdx.x, wmax);
}

}  // namespace mmt

using namespace mmt;

namespace {

const ConvKnobs& conv_knobs() {
  static const ConvKnobs k = conv_knobs_from_env();   // once per process
  return k;
}

// the pointers and flags of a launch's groups, checked and copied into a; ds: the fused downsamples' second sources
// (such a launch takes no residual and is not the pooled stem)
bool conv_groups(ConvF16Args& a, const mmt_conv_group* groups, const mmt_conv_ds* ds, int G) {
  if (!groups || G < 1 || G > kMaxGroups) return false;
  const int allowed = MMT_CONV_RELU | MMT_CONV_MAX | (ds ? 0 : MMT_CONV_POOL);
  for (int i = 0; i < G; ++i) {
    const mmt_conv_group& c = groups[i];
    if (!c.x || !c.w_hi || !c.w_lo || !c.y || !(c.w_scale > 0) || (c.flags & ~allowed) || (!c.x_max && !(c.x_scale > 0)) ||
        (c.flags & MMT_CONV_POOL) != (groups[0].flags & MMT_CONV_POOL) ||
        // the pooled stem kernel neither max-merges nor adds a residual: refuse operands it would drop
        ((c.flags & MMT_CONV_POOL) && ((c.flags & MMT_CONV_MAX) || c.resid)) ||
        (ds && (c.resid || !ds[i].x2 || (!ds[i].x2_max && !(ds[i].x2_scale > 0)))))
      return false;
    a.g[i] = ConvGroupArgs{c.x, c.w_hi, c.w_lo, c.bias, c.resid, c.y, c.x_max, c.y_max, c.x_scale, 1.0f / c.w_scale,
                           c.flags, ds ? ds[i].x2 : nullptr, ds ? ds[i].x2_max : nullptr, ds ? ds[i].x2_scale : 0.f};
  }
  // the twin layers of a grouped launch write disjoint outputs unless they merge (a MAX layer reads y)
  return !(G == 2 && (a.g[0].y == a.g[1].y || (a.g[0].flags | a.g[1].flags) & MMT_CONV_MAX));
}

// the plan's one launch, then the split-K reduce
int launch_plan(const ConvPlan& p, ConvF16Args& a, const ConvProblem& q, void* ws, hipStream_t s) {
  a.N = q.N; a.H = q.H; a.W = q.W; a.Cin = q.Cin; a.Cout = q.Cout; a.kh = q.kh; a.kw = q.kw; a.stride = q.stride;
  a.pad = q.pad; a.Ho = p.Ho; a.Wo = p.Wo; a.Kp = q.Kp; a.ks = p.ks;
  a.Cin2 = q.Cin2; a.H2 = q.H2; a.W2 = q.W2; a.stride2 = q.stride2;
  a.part = static_cast<float*>(ws);
  a.xcd_order = a.staged_epi = 1;
  const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(512);
  const bool wide = p.bn == 128;
  switch (p.kernel) {
    case ConvKernel::STEM_POOL:
      hipLaunchKernelGGL(conv_stem_pool_f16x3_kernel, grid, block, 0, s, a, p.PHo, p.PWo);
      break;
    case ConvKernel::PATCH:
      if (wide) hipLaunchKernelGGL(conv3x3_patch_f16x3_kernel<128>, grid, block, p.lds_bytes, s, a, p.tiles_per_img, p.patch_px);
      else hipLaunchKernelGGL(conv3x3_patch_f16x3_kernel<64>, grid, block, p.lds_bytes, s, a, p.tiles_per_img, p.patch_px);
      break;
    case ConvKernel::STEM:
      hipLaunchKernelGGL(conv_stem_f16x3_kernel, grid, block, 0, s, a);
      break;
    case ConvKernel::GENERIC:
      if (q.Cin <= 4) hipLaunchKernelGGL((conv_f16x3_kernel<64, true>), grid, block, 0, s, a);
      else if (wide) hipLaunchKernelGGL((conv_f16x3_kernel<128, false>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((conv_f16x3_kernel<64, false>), grid, block, 0, s, a);
      break;
    case ConvKernel::DEEP:
      if (wide) hipLaunchKernelGGL(conv_f16x3_deep_kernel<128>, grid, block, 0, s, a);
      else hipLaunchKernelGGL(conv_f16x3_deep_kernel<64>, grid, block, 0, s, a);
      break;
    case ConvKernel::NONE:
      return MMT_E_ARG;
  }
  if (p.reduce) {
    const int64_t n4 = (int64_t)q.N * p.Ho * p.Wo * q.Cout / 4;
    hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256), q.G), dim3(256), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? MMT_OK : MMT_E_HIP;
}

int conv_launch(const mmt_conv_group* groups, const mmt_conv_ds* ds, ConvProblem q, void* ws, size_t ws_bytes,
                void* stream) {
  ConvF16Args a{};
  if (!conv_groups(a, groups, ds, q.G)) return MMT_E_ARG;
  q.pool = groups[0].flags & MMT_CONV_POOL;
  q.ws_bytes = ws ? ws_bytes : 0;
  const ConvPlan p = conv_plan(q, conv_knobs());
  return p.error ? MMT_E_ARG : launch_plan(p, a, q, ws, (hipStream_t)stream);
}

}  // namespace

extern "C" {

size_t mmt_conv_max_words(void) { return (size_t)kMaxShards * kShardStride; }

size_t mmt_conv2d_f16x3_ws_bytes(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad,
                                 int groups) {
  const ConvProblem q{N, H, W, Cin, Cout, kh, kw, stride, pad, (int)conv_kp(Cin, kh, kw), groups, false, 0, 0, 0, 0, SIZE_MAX};
  return conv_plan(q, conv_knobs()).ws_needed;   // (0 for a rejected shape)
}

int mmt_conv2d_f16x3_groups(const mmt_conv_group* groups, int G, int N, int H, int W, int Cin, int Kp, int Cout,
                            int kh, int kw, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
  return conv_launch(groups, nullptr, ConvProblem{N, H, W, Cin, Cout, kh, kw, stride, pad, Kp, G, false, 0, 0, 0, 0, 0}, ws,
                     ws_bytes, stream);
}

int mmt_conv2d_f16x3_ds_groups(const mmt_conv_group* groups, const mmt_conv_ds* ds, int G, int N, int H, int W,
                               int Cin, int H2, int W2, int Cin2, int stride2, int Kp, int Cout, void* ws,
                               size_t ws_bytes, void* stream) {
  if (!ds || Cin2 <= 0) return MMT_E_ARG;   // (Cin2 > 0 is what tells the planner of the second source)
  return conv_launch(groups, ds, ConvProblem{N, H, W, Cin, Cout, 1, 1, 1, 0, Kp, G, false, Cin2, H2, W2, stride2, 0}, ws,
                     ws_bytes, stream);
}

int mmt_conv2d_f16x3(const float* x, int N, int H, int W, int Cin, const uint16_t* w_hi, const uint16_t* w_lo,
                     float w_scale, int Kp, const float* bias, int Cout, int kh, int kw, int stride, int pad,
                     const float* resid, float* y, const float* x_max, float x_scale, float* y_max, int flags,
                     void* stream) {
  const mmt_conv_group g{x, w_hi, w_lo, w_scale, bias, resid, y, x_max, x_scale, y_max, flags};
  return mmt_conv2d_f16x3_groups(&g, 1, N, H, W, Cin, Kp, Cout, kh, kw, stride, pad, nullptr, 0, stream);
}

}  // extern "C"
