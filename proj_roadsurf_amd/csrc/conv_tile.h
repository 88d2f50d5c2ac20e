// What the convolution kernels must agree on to give the same bits, stated once: the order in which tiles are handed out, the layout of
// a staged LDS row, the pixel decomposition, the fp16 clamp and hi / lo rounding, the order of the split mode's three products, and the
// epilogue of the tiled kernels.  conv_igemm / conv_deep / conv_wreg / conv_wide1x1_split / bneck_fused / bneck_split / stem_fused /
// conv_wgrad include it; their inner loops and schedules stay their own.  The integer and rounding parts also compile for the host
// (tests/test_conv_tile_cpu.py simulates the staging write against the fragment read over every lane).
//
// THE LDS ROW CONTRACT.  An operand row (one pixel, or one output channel) of a K step is 128 bytes = eight 16-byte chunks, staged by
// LDS-DMA: lane l of a wave writes slot lchk = l & 7 of row lrow = l >> 3 of the wave's 8-row piece, and the destination is lane-linear,
// so the swizzle is applied to the SOURCE: slot lchk of row r holds data chunk lchk ^ key(r) (src_chunk).
//   * fp16 form: data chunk d = K elements 8 d .. 8 d + 7 of the step's 64 (source offset chunk_f16).
//   * split form: a step covers 32 channels; chunks 0-3 are their hi halfs, 4-7 their lo halfs (chunk_split: the lo plane lies
//     `lo` elements behind the hi plane).
//   * activation rows: key = r & 7 (act_key).  Weight rows: key = (r & 3) | bit 2 from (r / blk) & 1 (w_key), where blk = 4 MI is
//     the number of consecutive rows one value of fi >> 2 reads (MI = 16-row blocks per wave: 16 for the 64-row wave tiles, 4 for the
//     16-row head tile, 4 MIB for the bottleneck's CBW-row matrices, 8 for conv_wide1x1_split's 32-row pass slices).
//   * the reader, lane (fi = l & 15, fq = l >> 4), takes for MFMA block i the row frag_row(fi, i, blk) = (fi >> 2) blk + 4 i + (fi & 3)
//     of its wave's rows (weights; which is the free channel permutation that leaves a lane with 4 MI consecutive channels), or row
//     16 j + fi (pixels).  Both have key == l & 7 = fkey whatever i or j: (row & 3) = fi & 3 and (row / blk) & 1 = (fi >> 2) & 1 as long
//     as 4 i + 3 < blk; (16 j + fi) & 7 = fi & 7.  So ONE per-lane constant undoes the swizzle: the fragment of half-step kk (fp16 form:
//     K elements 32 kk + 8 fq .. + 7; split form: kk = 0 the hi halfs, kk = 1 the lo halfs 8 fq .. + 7) sits at byte
//     frag_off(fq, fkey, kk) = ((4 kk + fq) ^ fkey) * 16 of the row.  Writer and reader agree because both go through the functions below.
// conv_wgrad.hip reads its rows transposed (ds_read_b64_tr_b16) and uses a different swizzle, row_key, which stays in that file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "common.h"
#define CT_D __device__ __forceinline__
#else
#define CT_D inline
#endif

// XCD-aware order: logical tile of position q among n.  Positions q and q + 8 share an XCD (L2) and get consecutive logical tiles; each
// XCD walks a contiguous run, so tiles that re-read one activation panel or neighbouring pixels hit the same L2.
CT_D int xcd_tile(int q, int n) {
  const int qn = n >> 3, r = n & 7, x = q & 7;
  return (x < r ? x * (qn + 1) : r * (qn + 1) + (x - r) * qn) + (q >> 3);
}

CT_D int act_key(int row) { return row & 7; }
CT_D int w_key(int row, int blk) { return (row & 3) | ((int)(((unsigned)row / (unsigned)blk) & 1u) << 2); }
CT_D int src_chunk(int lchk, int key) { return lchk ^ key; }
CT_D int chunk_f16(int d) { return d * 8; }                                                 // element offset inside the step's K
CT_D long long chunk_split(int d, long long lo) { return (d & 3) * 8 + (d >> 2) * lo; }
CT_D int frag_row(int fi, int i, int blk) { return (fi >> 2) * blk + i * 4 + (fi & 3); }
CT_D int frag_off(int fq, int fkey, int kk) { return ((4 * kk + fq) ^ fkey) * 16; }

// Pixel m of an (n, y, x)-ordered map.  pix_add: the same for m = m0 + r without a division, from the coordinates of m0 and of the
// offset r (rx < Wo, ry < Ho): one carry per digit suffices (conv_wreg's tile walk).
struct Pix { int x, y, n; };
CT_D Pix pix_of(int m, int Wo, int Ho) {
  const int t = m / Wo;
  return Pix{m % Wo, t % Ho, t / Ho};
}
CT_D Pix pix_add(int x0, int y0, int n0, int rx, int ry, int rn, int Wo, int Ho) {
  int x = x0 + rx;
  const int cx = x >= Wo;
  x -= cx ? Wo : 0;
  int y = y0 + ry + cx;
  const int cy = y >= Ho;
  y -= cy ? Ho : 0;
  return Pix{x, y, n0 + rn + cy};
}

#if !defined(CT_NO_F16)
#if !defined(__HIPCC__)
typedef _Float16 half_t;
#endif
// The clamp in front of every fp16 rounding (common.h: saturation counting).  A NaN passes through both forms.  After a ReLU only the
// upper bound matters; the two forms differ for f < -65504, so both exist.
CT_D float clamp_h16(float f) { return f > 65504.f ? 65504.f : (f < -65504.f ? -65504.f : f); }
CT_D float clamp_h16_pos(float f) { return f > 65504.f ? 65504.f : f; }
// x = hi + lo of the split-operand mode: hi = fp16(f), lo = fp16(f - hi), both round-to-nearest-even.  By value.
struct HiLo { half_t h, l; };
CT_D HiLo split_round(float f) {
  const half_t h = (half_t)f;
  return HiLo{h, (half_t)(f - (float)h)};
}
#endif

#if defined(__HIPCC__)
// 16 bytes per lane, global -> LDS without a register round trip: lane l's 16 bytes land at lds_wave_base + 16 l
__device__ __forceinline__ void glds16(const half_t* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Rows of a launch bounded by a device counter: min(M, *m_count * m_mul).  P: ConvParams or WgradParams.
template <class P>
__device__ __forceinline__ int conv_rows(const P& p) {
  int M = p.M;
  if (p.m_count) {
    const long long mc = (long long)(*p.m_count) * p.m_mul;
    if (mc < M) M = (int)mc;
  }
  return M;
}

// The split mode's three products of one K step in the one order every tile uses (W_hi.X_lo, W_hi.X_hi, W_lo.X_hi into one accumulator;
// lo.lo is dropped), so that an output's bits do not depend on the tile that computed it.  Kernels that interleave other work between the
// products (conv_deep's split loop, conv_wide1x1_split) place them by hand in this order.
// (By reference: with the accumulator passed and returned by value hipcc unrolled bneck_split's conv2 loop in full, 40 % more code.)
__device__ __forceinline__ void mfma_split3(f32x4& acc, const half8& wh, const half8& wl, const half8& xh, const half8& xl) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
}

// Exponent of a tensor-wide power-of-two scale from the abs-max pass's two device words (bits of the largest finite |v|, non-finite flag):
// e = 14 - floor(log2 amax), so that the scaled maximum lies in [2^14, 2^15); 0 for an all-zero or a non-finite tensor.  The split weight
// gradient (conv_wgrad.hip) and the split input gradient (epi_values_dgrad_split below) read it behind the pass, on the device.
__device__ __forceinline__ int split_tensor_exp(unsigned amax_bits, unsigned nonfinite) {
  if (nonfinite || amax_bits == 0) return 0;
  const int be = (int)(amax_bits >> 23);
  const int E = be ? be - 127 : (31 - __clz((int)amax_bits)) - 149;     // floor(log2(amax)), subnormal fp32 included
  return 14 - E;
}

// ---- the epilogue of conv_igemm_kernel and conv_deep_tile: a lane holds channels crow .. crow + 4 MI - 1 of one pixel per 16-pixel block.
// Saturation counting stays with the caller (a screen in conv_igemm, a per-lane counter in conv_deep: common.h) through epi_store_h16's functor.
template <int MI, bool SPLIT>
struct EpiRows {
  float bias[4 * MI];
  float wsc[SPLIT ? 4 * MI : 1];     // per-row weight descale of the split mode
};
template <int MI, bool SPLIT>
__device__ __forceinline__ EpiRows<MI, SPLIT> epi_rows(const float* bias, const float* wscale, int crow) {
  EpiRows<MI, SPLIT> rw;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const f32x4 b4 = *(const f32x4*)(bias + crow + i * 4);
    rw.bias[i * 4 + 0] = b4[0]; rw.bias[i * 4 + 1] = b4[1]; rw.bias[i * 4 + 2] = b4[2]; rw.bias[i * 4 + 3] = b4[3];
  }
  if constexpr (SPLIT) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x4 s4 = *(const f32x4*)(wscale + crow + i * 4);
      rw.wsc[i * 4 + 0] = s4[0]; rw.wsc[i * 4 + 1] = s4[1]; rw.wsc[i * 4 + 2] = s4[2]; rw.wsc[i * 4 + 3] = s4[3];
    }
  }
  return rw;
}

// v = acc * wscale + bias (acc + bias), then the addends in their fixed order: residual, FPN top-down (coarser map at (y / 2, x / 2)),
// TRAIN: the 2x2 sum of the finer gradient map, the fp32 addend, the ReLU-backward mask; then ReLU.  (x, y, n): the pixel; opix: its
// position in the output's geometry (which res / res32 / mask share); cb: the lane's first channel.
template <int MI, int NJ, bool TRAIN, bool SPLIT>
__device__ __forceinline__ void epi_values(float (&v)[4 * MI], const ConvParams& p, const f32x4 (&acc)[MI][NJ], const int j, const EpiRows<MI, SPLIT>& rw,
                                           const long long opix, const int cb, const int x, const int y, const int n) {
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (SPLIT) v[i * 4 + r] = acc[i][j][r] * rw.wsc[i * 4 + r] + rw.bias[i * 4 + r];
      else v[i * 4 + r] = acc[i][j][r] + rw.bias[i * 4 + r];
    }
  // an fp16 addend (hi + lo planes in the split mode) at element pointer a
  auto add_h16 = [&](const half_t* a, const long long lo) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const half4 h = *(const half4*)(a + i * 4);
      if constexpr (SPLIT) {
        const half4 l = *(const half4*)(a + lo + i * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[i * 4 + r] += (float)h[r] + (float)l[r];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[i * 4 + r] += (float)h[r];
      }
    }
  };
  if (p.res) add_h16(p.res + opix * p.out_Cs + cb, p.res_lo);
  if (p.up) {
    const long long upix = (long long)(n * p.up_Hp + (y >> 1) + p.up_pad) * p.up_Wp + (x >> 1) + p.up_pad;
    add_h16(p.up + upix * p.up_Cs + cb, p.up_lo);
  }
  if (TRAIN && p.down) {      // backward of the nearest 2x upsample: add the 2x2 block of the finer gradient map
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
      const long long dpix = (long long)(n * p.down_Hp + 2 * y + (dd >> 1) + p.down_pad) * p.down_Wp + 2 * x + (dd & 1) + p.down_pad;
      const half_t* dp = p.down + dpix * p.down_Cs + cb;
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const half4 h = *(const half4*)(dp + i * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[i * 4 + r] += (float)h[r];
      }
    }
  }
  if (TRAIN && p.res32) {
    const float* rp = p.res32 + opix * p.out_Cs + cb;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x4 h = *(const f32x4*)(rp + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i * 4 + r] += h[r];
    }
  }
  if (TRAIN && p.mask) {      // ReLU backward
    const half_t* mp = p.mask + opix * p.out_Cs + cb;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const half4 h = *(const half4*)(mp + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i * 4 + r] = (float)h[r] > 0.f ? v[i * 4 + r] : 0.f;
    }
  }
  if (p.relu) {
#pragma unroll
    for (int e = 0; e < 4 * MI; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
  }
}

// Third flavour, the fp32 trainer's input gradient on split operands (ConvParams::dy_amax set; conv_igemm's TRAIN && SPLIT instantiation):
// v = acc * wscale[row] * 2^-e_dy with e_dy from the device words behind the abs-max pass, then the fp32 addends in ref_f32.hip's order --
// res, the 2x2 sum of `down`, res32 -- then the ReLU-backward mask (fp32 saved activation, > 0).  No bias: the product has none.
template <int MI, int NJ>
__device__ __forceinline__ void epi_values_dgrad_split(float (&v)[4 * MI], const ConvParams& p, const f32x4 (&acc)[MI][NJ], const int j, const EpiRows<MI, true>& rw,
                                                       const int e_dy, const long long opix, const int cb, const int x, const int y, const int n) {
#pragma unroll
  for (int e = 0; e < 4 * MI; ++e) v[e] = ldexpf(acc[e >> 2][j][e & 3] * rw.wsc[e], -e_dy);      // both factors are powers of two
  auto add_f32 = [&](const float* a) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x4 h = *(const f32x4*)(a + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i * 4 + r] += h[r];
    }
  };
  if (p.res) add_f32((const float*)p.res + opix * p.out_Cs + cb);
  if (p.down) {
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
      const long long dpix = (long long)(n * p.down_Hp + 2 * y + (dd >> 1) + p.down_pad) * p.down_Wp + 2 * x + (dd & 1) + p.down_pad;
      add_f32((const float*)p.down + dpix * p.down_Cs + cb);
    }
  }
  if (p.res32) add_f32(p.res32 + opix * p.out_Cs + cb);
  if (p.mask) {
    const float* mp = (const float*)p.mask + opix * p.out_Cs + cb;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x4 h = *(const f32x4*)(mp + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i * 4 + r] = h[r] > 0.f ? v[i * 4 + r] : 0.f;
    }
  }
}

// Fourth flavour, the fp32 trainer's forward product on split operands (ConvParams::x_amax set; conv_igemm's TRAIN && SPLIT instantiation with FWD):
// v = acc * wscale[row] * 2^-e_x with e_x from the device words behind the abs-max pass of X, then in ref_f32.hip's order the fp32 bias,
// the fp32 residual, the fp32 FPN top-down addend at (y >> 1, x >> 1), and ReLU.  rw.bias holds the bias here.
template <int MI, int NJ>
__device__ __forceinline__ void epi_values_fwd_split(float (&v)[4 * MI], const ConvParams& p, const f32x4 (&acc)[MI][NJ], const int j, const EpiRows<MI, true>& rw,
                                                     const int e_x, const long long opix, const int cb, const int x, const int y, const int n) {
#pragma unroll
  for (int e = 0; e < 4 * MI; ++e) v[e] = ldexpf(acc[e >> 2][j][e & 3] * rw.wsc[e], -e_x) + rw.bias[e];      // both factors are powers of two
  auto add_f32 = [&](const float* a) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const f32x4 h = *(const f32x4*)(a + i * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[i * 4 + r] += h[r];
    }
  };
  if (p.res) add_f32((const float*)p.res + opix * p.out_Cs + cb);
  if (p.up) {
    const long long upix = (long long)(n * p.up_Hp + (y >> 1) + p.up_pad) * p.up_Wp + (x >> 1) + p.up_pad;
    add_f32((const float*)p.up + upix * p.up_Cs + cb);
  }
  if (p.relu) {
#pragma unroll
    for (int e = 0; e < 4 * MI; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
  }
}

template <int MI>
__device__ __forceinline__ void epi_store_f32(float* op, const float (&v)[4 * MI]) {
#pragma unroll
  for (int i = 0; i < MI; ++i) *(f32x4*)(op + i * 4) = f32x4{v[i * 4], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]};
}

// clamp, round to fp16 (SPLIT: hi and lo planes, the lo plane out_lo elements behind): one 16-byte store per 8 channels and plane, 8-byte
// stores for an odd MI.  count(unclamped, clamped) sees every element on its way: the caller's saturation counting.
template <int MI, bool SPLIT, class F>
__device__ __forceinline__ void epi_store_h16(half_t* op, const long long out_lo, const float (&v)[4 * MI], F&& count) {
  constexpr int W = MI % 2 == 0 ? 8 : 4;
  typedef _Float16 hvec __attribute__((ext_vector_type(W)));
#pragma unroll
  for (int c = 0; c < 4 * MI; c += W) {
    hvec h, l;
#pragma unroll
    for (int r = 0; r < W; ++r) {
      const float f = clamp_h16(v[c + r]);
      count(v[c + r], f);
      const HiLo s = split_round(f);
      h[r] = s.h;
      l[r] = s.l;
    }
    *(hvec*)(op + c) = h;
    if constexpr (SPLIT) *(hvec*)(op + out_lo + c) = l;
  }
}
#endif
