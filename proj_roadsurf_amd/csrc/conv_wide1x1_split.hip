// 1x1 convolution with K = 256 and many output rows in the SPLIT-OPERAND precision mode (common.h ConvParams::split): a workgroup owns a tile of pixels and
// produces ALL rows for them.  conv_igemm / conv_deep tile such a layer 256 rows at a time: with 1024 rows every pixel tile is staged four times, each time
// behind an eight-step K loop whose fill and drain cost as much as the steps.  Here the pixels never pass through LDS:
//
//   * every wave loads its NJ x 16 pixels' 256 channels, hi and lo planes, ONCE, straight into MFMA B fragments -- lane (fi, fq) of K step s holds the
//     16 bytes at channel 32 s + 8 fq of pixel fi from each plane: 8 steps x NJ blocks x 2 planes x 4 = 64 NJ registers;
//   * the weight matrix goes by in passes of 32 rows, a slice of [8 K steps][32 rows][32 hi | 32 lo halfs] = 32 KB staged by LDS-DMA with conv_igemm's
//     swizzle, double buffered: slice n + 1 is requested a piece per K step under the MFMAs of pass n (64 KB of LDS, two workgroups per CU).  The compiler
//     waits vmcnt(0) in front of every pass's epilogue for the bias / scale / predictor loads, which also retires that slice and the next residual: by then
//     they have had the pass's MFMAs to land, but only the epilogue's STORES outlive a pass;
//   * the form is the conv3 phase of bneck_split.hip with the B operand from HBM instead of from conv2's accumulators.
//
// Same bits as every other split tile: K steps in ascending order, per step W_hi.X_lo, W_hi.X_hi, W_lo.X_hi into one accumulator, conv_igemm's k-to-lane
// mapping.  Two passes make one 64-row block of conv_igemm's MI = 4 wave tile: pass 2 P + h holds its accumulators i = 2 h, 2 h + 1, so lane (fi, fq) ends up with
// channels 64 P + 16 fq + 8 h .. + 7 of pixel fi -- one 16-byte store per plane.
//
// Epilogues, term for term conv_igemm's SPLIT paths:
//   mode 0: acc * wscale + bias, + (res_hi + res_lo), ReLU, clamp with the saturation screen, hi = fp16(v), lo = fp16(v - hi).  The residual of pass n + 1 is
//           loaded before the MFMAs of pass n.  A 64-row block is stored after its second pass, and those stores stay in flight over the wait at the top of
//           the following pass (counted vmcnt: they are the youngest vector-memory operations of the wave; everything older has been waited for by the
//           compiler's vmcnt(0) in front of the epilogue, so the counted wait can never wait for too little).
//   mode 2: the fused mask predictor (deconv 2x2 s2 + ReLU + the predicted class' 1x1).  The per-lane dot runs over the 16 channels of a 64-row block in
//           ascending order across its two passes, then __shfl_xor 16 and 32 -- one "channel wave" of the 128x256 tile; the four blocks of a (dy, dx)
//           group are summed ((P0 + P1) + P2) + P3 as that tile sums its channel waves, in registers, and the logit is STORED: no LDS round trip, no atomic, and
//           the logits need no zeroing (every word of an entry below the device-side count is written; the others are never read).
#include "conv_tile.h"

namespace {

constexpr int PR = 32;                    // weight rows per pass
constexpr int KS = 8;                     // K steps of 32 channels
constexpr int SLICE = KS * PR * 128;      // 32 KB
constexpr int LDS_BYTES = 2 * SLICE;

// One term of the predictor's dot, as the 128x256 tile's COMPILED code rounds it (the logits must carry its bits): the first four channels of a 64-row block are
// fused multiply-adds, the other twelve are rounded products added one by one.  That is what hipcc makes of `sdot += v * w` in conv_igemm.hip's split
// instantiation (noted there); the bit-equality test against variant 14 is what notices when the two part.
__device__ __forceinline__ float dot_term(float s, float v, float w, bool fused) {
  if (fused) return __builtin_fmaf(v, w, s);
  {
#pragma clang fp contract(off)
    const float m = v * w;
    return s + m;
  }
}

template <int NW, int NJ, int MODE>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void conv_wide1x1_split_kernel(const ConvParams p) {
  constexpr int BM = NW * NJ * 16;
  constexpr int NG = 32 / NW;               // LDS-DMA pieces (8 rows of one K step) per wave and slice
  constexpr int ST = MODE == 2 ? NJ : 4 * NJ;   // stores a full wave issues in a storing pass
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = conv_rows(p);
  const int ntiles = (M + BM - 1) / BM;
  const int q = blockIdx.x;
  if (q >= ntiles) return;                  // the grid comes from the capacity: nothing is touched past the device-side count
  const int m0 = xcd_tile(q, ntiles) * BM;      // neighbouring tiles share an L2
  const int rows = p.Cout * (MODE == 2 ? 4 : 1);
  const int npass = rows / PR;

  // ---- weight slices: piece k of a wave = rows 8 rp .. + 7 of K step k * (NW / 4) + s0; LDS row l = 8 rp + lrow of a slice holds weight row
  //      64 P + 8 h + 16 rp + lrow, which is row (fi >> 2) * 16 + (2 h + ii) * 4 + (fi & 3) of conv_igemm's 64-row block for the reader l = (fi >> 2) * 8 + ii * 4 + (fi & 3)
  const int lrow = lane >> 3, lchk = lane & 7;
  const int rp = wave & 3, s0 = wave >> 2;
  const half_t* wsrc;
  {
    const int d = src_chunk(lchk, w_key(8 * rp + lrow, 8));     // data chunk of LDS slot lchk of slice row 8 rp + lrow (conv_tile.h: block height 8)
    wsrc = p.w + (long long)(rp * 16 + lrow) * p.Kpad + s0 * 32 + chunk_split(d, p.w_lo);
  }
  auto stage_piece = [&](int pass, int k) {
    const half_t* g = wsrc + (long long)((pass >> 1) * 64 + (pass & 1) * 8) * p.Kpad;
    char* base = smem + (pass & 1) * SLICE + (s0 * PR + rp * 8) * 128;
    glds16(g + k * (NW / 4) * 32, base + k * (NW / 4) * PR * 128);
  };

  const int fi = lane & 15, fq = lane >> 4, fkey = lane & 7;
  int w_off[2];
#pragma unroll
  for (int ii = 0; ii < 2; ++ii) w_off[ii] = frag_row(fi, ii, 8) * 128;
  const int ch_off = frag_off(fq, fkey, 0), cl_off = frag_off(fq, fkey, 1);    // this lane's hi / lo fragment inside a row

  // ---- this wave's pixels: B fragments of all eight K steps, both planes
  half8 xh[KS][NJ], xl[KS][NJ];
  bool valid[NJ];
  long long opix[NJ];            // mode 0: output pixel; mode 2: word of the entry's (2 y, 2 x) logit
  const float* wv[NJ];           // mode 2: predictor weights of the entry's class
  const bool full = m0 + (wave + 1) * NJ * 16 <= M;      // wave-uniform: every store below is issued
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int m = m0 + (wave * NJ + j) * 16 + fi;
    valid[j] = m < M;
    const int mm = valid[j] ? m : M - 1;
    const Pix px = pix_of(mm, p.Wo, p.Ho);
    const int x = px.x, y = px.y, n = px.n;
    const half_t* xp = p.in + ((long long)(n * p.in_Hp + y + p.in_off) * p.in_Wp + x + p.in_off) * 256 + fq * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) { xh[s][j] = *(const half8*)(xp + s * 32); xl[s][j] = *(const half8*)(xp + p.in_lo + s * 32); }
    if (MODE == 2) {
      const int slot = p.dot_slot[n];
      wv[j] = p.dot_w + (long long)p.dot_cls[slot] * p.Cout;
      opix[j] = (long long)slot * (4 * p.Ho * p.Wo) + (long long)(2 * y) * (2 * p.Wo) + 2 * x;
    } else {
      wv[j] = nullptr;
      opix[j] = (long long)(n * p.out_Hp + y + p.out_pad) * p.out_Wp + x + p.out_pad;
    }
  }
  const bool has_res = MODE == 0 && p.res != nullptr;
  half8 rh[NJ], rl[NJ], qh[NJ], ql[NJ];      // residual of the pass being computed and of the next one, loaded one pass ahead
  auto load_res = [&](int pass, half8* h, half8* l) {
    const int c = (pass >> 1) * 64 + fq * 16 + (pass & 1) * 8;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const half_t* rp2 = p.res + opix[j] * p.out_Cs + c;
      h[j] = *(const half8*)rp2;
      l[j] = *(const half8*)(rp2 + p.res_lo);
    }
  };
#pragma unroll
  for (int j = 0; j < NJ; ++j) { rh[j] = half8{0, 0, 0, 0, 0, 0, 0, 0}; rl[j] = rh[j]; qh[j] = rh[j]; ql[j] = rh[j]; }
#pragma unroll
  for (int k = 0; k < NG; ++k) stage_piece(0, k);
  if (has_res) load_res(0, rh, rl);

  // The pass loop waits by hand; a use the compiler can see, here, makes it wait for the fragment loads once instead of before the first MFMA of every
  // loop trip (which would drain the slice just put in flight).
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(xh[s][j]), "v"(xl[s][j]));
  float sdot[NJ], gsum[NJ];
  half8 kh[MODE == 0 ? NJ : 1], kl[MODE == 0 ? NJ : 1];      // mode 0: an even pass's output halves, kept for the odd pass's stores
#pragma unroll
  for (int j = 0; j < NJ; ++j) { sdot[j] = 0.f; gsum[j] = 0.f; }
  int pend = 0;                  // stores this wave issued in the previous pass (0 = none, or not known exactly)
  // one pass; `ch / cl` hold its residual, `nh / nl` receive the next pass's.  Called twice per loop trip with the two register sets swapped, so that no copy
  // (and with it no wait for the loads just issued) stands at the end of a pass.
  auto run_pass = [&](const int pass, half8 (&ch)[NJ], half8 (&cl)[NJ], half8 (&nh)[NJ], half8 (&nl)[NJ]) __attribute__((always_inline)) {
    // Slice `pass` (and the residual of this pass) must have landed; the previous pass's stores are younger than both and are not waited for.  vmcnt counts
    // loads, stores and LDS-DMA in issue order.  __syncthreads() would drain the stores (its fence waits vmcnt(0)), hence the raw barrier; it also ends every
    // wave's fragment reads of the buffer that is restaged next.
    if (pend) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(ST) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = pass + 1 < npass;
    if (more && has_res) load_res(pass + 1, nh, nl);
    // epilogue operands of this pass, requested ahead of their use: under the MFMAs of the last two K steps (earlier, 256 registers do not hold them)
    const int crow = (pass >> 1) * 64 + fq * 16 + (pass & 1) * 8;
    const int g = MODE == 2 ? crow / p.Cout : 0, cb = crow - g * p.Cout;
    float bias[8], wsc[8];
    float dw[MODE == 2 ? NJ : 1][8];
    auto load_epi = [&]() {
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const f32x4 b4 = *(const f32x4*)(p.bias + crow + ii * 4), s4 = *(const f32x4*)(p.wscale + crow + ii * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) { bias[ii * 4 + r] = b4[r]; wsc[ii * 4 + r] = s4[r]; }
      }
      if (MODE == 2) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int ii = 0; ii < 2; ++ii) {
            const f32x4 w4 = *(const f32x4*)(wv[j] + cb + ii * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) dw[j][ii * 4 + r] = w4[r];
          }
      }
    };
    __builtin_amdgcn_sched_barrier(0);      // keep the requests above the matrix work (the scheduler would sink them to their use)
    const char* sb = smem + (pass & 1) * SLICE;
    f32x4 acc[2][NJ];
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[ii][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Weight fragments one step ahead of the MFMAs that use them, in three rotating sets: W_hi of step s + 1 is requested before the W_hi blocks of step s,
    // W_lo of step s + 1 after the W_lo block of step s has read its registers.  One wave per SIMD has nothing else to cover the LDS latency with; the
    // sched_barriers keep the scheduler from moving the requests back down to their use.
    auto frag = [&](int s, int ii, int off) { return *(const half8*)(sb + s * (PR * 128) + w_off[ii] + off); };
    half8 wh[2], wl[2], nwh[2];
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) { wh[ii] = frag(0, ii, ch_off); wl[ii] = frag(0, ii, cl_off); }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s + 1 < KS) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) nwh[ii] = frag(s + 1, ii, ch_off);
      }
      if (s == KS - 2) load_epi();
      // the next slice, two pieces per K step from the first on: an LDS-DMA piece costs the wave tens of cycles to issue, which the MFMAs cover, and the
      // last one has landed long before the wait in front of the epilogue
      if (more && 2 * s < NG) { stage_piece(pass + 1, 2 * s); stage_piece(pass + 1, 2 * s + 1); }
      __builtin_amdgcn_sched_barrier(0);
      // the three products in mfma_split3's order (conv_tile.h owns it), placed by hand round the sched_barriers
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ii], xl[s][j], acc[ii][j], 0, 0, 0);
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ii], xh[s][j], acc[ii][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ii], xh[s][j], acc[ii][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (s + 1 < KS) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) { wl[ii] = frag(s + 1, ii, cl_off); wh[ii] = nwh[ii]; }
      }
    }

    // ---- epilogue: lane holds rows crow .. crow + 7 of pixel (j, fi)
    if (MODE == 2) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float v[8];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[ii * 4 + r] = acc[ii][j][r] * wsc[ii * 4 + r] + bias[ii * 4 + r];
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        float sd = sdot[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) sd = dot_term(sd, v[e], dw[j][e], (pass & 1) == 0 && e < 4);
        sdot[j] = sd;
      }
      pend = 0;
      if (pass & 1) {            // a 64-row block is complete: one channel wave of the 128x256 tile
        const int blocks = p.Cout >> 6, k = (pass >> 1) % blocks;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          float v0 = sdot[j];
          v0 += __shfl_xor(v0, 16);
          v0 += __shfl_xor(v0, 32);
          gsum[j] = k == 0 ? v0 : gsum[j] + v0;
          sdot[j] = 0.f;
        }
        if (k == blocks - 1) {
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            if (fq == 0 && valid[j]) p.dot_out[opix[j] + (long long)(g >> 1) * (2 * p.Wo) + (g & 1)] = gsum[j];
          pend = full ? ST : 0;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float v[8];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[ii * 4 + r] = acc[ii][j][r] * wsc[ii * 4 + r] + bias[ii * 4 + r];
        if (has_res) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += (float)ch[j][e] + (float)cl[j][e];
        }
        if (p.relu) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
        }
        // saturation screen (common.h rs_sat_bad): the sum of |clamped value| is NaN or >= 65504 whenever an element is NaN or out of range
        float scr = 0.f;
        half8 h, l;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = clamp_h16(v[e]);
          scr += __builtin_fabsf(f);
          const HiLo hl = split_round(f);
          h[e] = hl.h;
          l[e] = hl.l;
        }
        if (valid[j] && !(scr < 65504.f)) {     // rare: count exactly
          unsigned c = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) c += rs_sat_bad(v[e]);
          rs_sat_flush(p.sat, c);
        }
        // the two passes of a 64-row block are stored together: 32 contiguous bytes per lane and plane, as conv_igemm's wave tile writes them
        if ((pass & 1) == 0) {
          kh[j] = h; kl[j] = l;
        } else if (valid[j]) {
          half_t* op = (half_t*)p.out + opix[j] * p.out_Cs + crow - 8;
          *(half8*)op = kh[j];
          *(half8*)(op + 8) = h;
          *(half8*)(op + p.out_lo) = kl[j];
          *(half8*)(op + p.out_lo + 8) = l;
        }
      }
      pend = (pass & 1) && full ? ST : 0;
    }
  };
  for (int pass = 0; pass < npass; pass += 2) {      // rows % 64 == 0: an even number of passes
    run_pass(pass, rh, rl, qh, ql);
    run_pass(pass + 1, qh, ql, rh, rl);
  }
}

template <int NW, int NJ>
int launch_px(const ConvParams& p, hipStream_t stream) {
  const long long nblk = cdiv(p.M, NW * NJ * 16);
  RS_CHECK(nblk > 0 && nblk < (1ll << 31), RS_ERR_ARG, "conv_wide1x1_split: bad grid %lld", nblk);
  const void* k = p.mode == 2 ? (const void*)conv_wide1x1_split_kernel<NW, NJ, 2> : (const void*)conv_wide1x1_split_kernel<NW, NJ, 0>;
  static bool attr[2] = {false, false};
  const int ai = p.mode == 2 ? 1 : 0;
  if (!attr[ai]) {
    RS_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr[ai] = true;
  }
  ConvParams pc = p;
  void* args[] = {&pc};
  RS_HIP(hipLaunchKernel(k, dim3((unsigned)nblk), dim3(NW * 64), args, LDS_BYTES, stream));
  return RS_OK;
}

}  // namespace

// The shapes the kernel takes (pointers are checked at launch): split operands, 1x1, stride 1, one K source of exactly 256 channels at pitch 256, rows a
// multiple of 64, plain fp16-plane output (mode 0) or the fused mask predictor over groups of 256 channels (mode 2)
bool conv_wide1x1_split_ok(const ConvParams& p) {
  const int rows = p.Cout * (p.mode != 0 ? 4 : 1);
  return p.split && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.Cin == 256 && p.in_Cs == 256 && p.Kpad >= 256 && !p.in2 && !p.up && !p.out_f32 &&
         !p.koff && !p.head_w && p.nseg == 0 && !p.down && !p.res32 && !p.mask && p.out_stride <= 1 && rows > 0 && rows % 64 == 0 &&
         (p.mode == 0 || (p.mode == 2 && p.Cout == 256)) &&
         // 16-byte vector accesses: pitches and plane offsets in whole groups of 8 halfs, an output pixel wide enough for all rows
         p.Kpad % 8 == 0 && p.in_lo % 8 == 0 && p.w_lo % 8 == 0 &&
         (p.mode != 0 || (p.out_Cs % 8 == 0 && p.out_Cs >= rows && p.out_lo % 8 == 0 && p.res_lo % 8 == 0));
}

int launch_conv_wide1x1_split(const ConvParams& p, hipStream_t stream, int tile_px) {
  RS_CHECK(conv_wide1x1_split_ok(p), RS_ERR_UNSUPPORTED, "conv_wide1x1_split: takes split-operand 1x1 / stride 1 / Cin 256 layers with rows %% 64 == 0 (mode 0, or mode 2 with Cout 256)");
  RS_CHECK(p.M > 0 && p.in && p.w && p.bias && p.wscale && (!p.m_count || p.m_mul > 0), RS_ERR_ARG, "conv_wide1x1_split: null argument");
  if (p.mode == 2) RS_CHECK(p.dot_w && p.dot_cls && p.dot_slot && p.dot_out, RS_ERR_ARG, "conv_wide1x1_split: the fused mask predictor needs its pointers");
  else RS_CHECK(p.out, RS_ERR_ARG, "conv_wide1x1_split: null output");
  switch (tile_px) {
    case 64: return launch_px<4, 1>(p, stream);
    case 128: return launch_px<4, 2>(p, stream);
    case 256: return launch_px<8, 2>(p, stream);
    default: rs_set_error("conv_wide1x1_split: tile of %d pixels (64, 128 or 256)", tile_px); return RS_ERR_ARG;
  }
}
