// ROIPooler + ROIAlign(aligned=True, sampling_ratio=0) of the Mask R-CNN forward and its backward for the trainer, gfx950.  Which level, which
// samples, which weights: roi_geom.h, once for all five kernels; this file is what they do with features and gradients.  Compiled with
// -ffp-contract=off like the rest of the detection glue (torchvision's fp32 operation order).
//   roi_align_kernel        per-sample form, torchvision's summation order (fp32 validation mode, RS_ROI_WINDOW=0)
//   roi_align_win_kernel    separable per-bin weight tables, every cell of a bin's window read once (fp16 and split-operand modes)
//   roi_align_bwd_kernel    adjoint of the windowed form by float atomics (RS_ROI_BWD_ATOMIC=1, and the RoIs too large for the tables)
//   roi_bwd_prep_kernel / roi_bwd_gather_kernel   owner-computes backward: per-entry tables, then one workgroup per 8 x 8-cell region
// [EXT d2: modeling/poolers.py; EXT tv: csrc/ops/cuda/roi_align_kernel.cu]
#include <cstddef>

#include "detect.h"
#include "roi_geom.h"

namespace {

// ---------------------------------------------------------------------------------------------
// ROIAlign (aligned = true, adaptive sampling), C == 256, one workgroup per RoI.
// Phase 1: the P*gh row samples and P*gw column samples of the RoI are computed ONCE (address
// offset of the low/high neighbour + the two interpolation weights, zero weights for samples the
// reference skips) into LDS.  Phase 2: each half-wave owns one bin at a time; a lane carries 8
// consecutive channels (16-byte loads, 512 contiguous bytes per half-wave per neighbour), so the
// per-sample VALU work is 4 weight products + 32 multiply/adds instead of the full coordinate
// arithmetic.  Operation order of the accumulation follows torchvision's kernel exactly.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roi_align_kernel(const RoiAlignParams p) {
  __shared__ int s_lo[2][RS_ROI_MAXS], s_hi[2][RS_ROI_MAXS];     // [0] = y (row offsets), [1] = x (column offsets), in elements
  __shared__ float s_l[2][RS_ROI_MAXS], s_h[2][RS_ROI_MAXS];
  const int entry = blockIdx.x;
  const int tid = threadIdx.x;
  int slot, n;
  const int kind = roi_entry(p, entry, slot, n);
  if (kind == 0) return;
  const int P = p.P, PP = P + 2 * p.out_pad;
  const int es = p.f32 == 1 ? 4 : 2;            // element size of features / output (p.f32 == 2: split-operand mode, two fp16 planes)
  char* out = (char*)p.out + (long long)entry * PP * PP * 256 * es;
  const int hw = tid >> 5, l32 = tid & 31;       // half-wave id, lane inside it (8 channels each)
  if (kind == 1) {
    for (int b = hw; b < P * P; b += 8) {
      const int ph = b / P, pw = b - ph * P;
      char* o = out + (((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) * es;
      if (p.f32 == 1) { ((f32x4*)o)[0] = f32x4{0.f, 0.f, 0.f, 0.f}; ((f32x4*)o)[1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      else { half8 z; for (int i = 0; i < 8; ++i) z[i] = (half_t)0.f; *(half8*)o = z; if (p.f32 == 2) *(half8*)(o + p.out_lo * 2) = z; }
    }
    return;
  }
  const float* r = p.rois + (long long)slot * 4;
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const int lvl = roi_level(x1, y1, x2, y2, p.nlevels);
  if (p.out_level) { if (tid == 0) p.out_level[entry] = lvl; }
  const int H = p.H[lvl], W = p.W[lvl];
  const float sc = p.scale[lvl];
  const char* feat = (const char*)p.feat[lvl] + ((long long)n * (H + 2) * (W + 2) * 256 + l32 * 8) * es;
  const RoiBins rb = roi_bins(x1, y1, x2, y2, sc, P);
  const int gh = rb.gh, gw = rb.gw;
  const float count = rb.count;
  const bool fast = (P * gh <= RS_ROI_MAXS) && (P * gw <= RS_ROI_MAXS);

  // one sample coordinate -> (low offset, high offset, l, h); out-of-range samples get zero weights
  auto prep = [&](float c, int size, int pitch, int& lo, int& hi, float& l, float& h) {
    const RoiSample s = roi_sample(c, size);
    l = s.l;
    h = s.h;
    lo = (s.lo + 1) * pitch;
    hi = (s.hi + 1) * pitch;
  };
  if (fast) {
    for (int t = tid; t < P * gh; t += 256) {
      const int ph = t / gh, iy = t - ph * gh;
      prep(roi_coord(rb.start_h, rb.bin_h, ph, iy, gh), H, (W + 2) * 256, s_lo[0][t], s_hi[0][t], s_l[0][t], s_h[0][t]);
    }
    for (int t = tid; t < P * gw; t += 256) {
      const int pw = t / gw, ix = t - pw * gw;
      prep(roi_coord(rb.start_w, rb.bin_w, pw, ix, gw), W, 256, s_lo[1][t], s_hi[1][t], s_l[1][t], s_h[1][t]);
    }
  }
  __syncthreads();
  for (int b0 = 0; b0 < P * P; b0 += 8) {
    const int b = b0 + hw;
    const bool live = b < P * P;
    const int bb = live ? b : P * P - 1;
    const int ph = bb / P, pw = bb - ph * P;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    for (int iy = 0; iy < gh; ++iy) {
      int ylo, yhi; float ly, hy;
      if (fast) { const int t = ph * gh + iy; ylo = s_lo[0][t]; yhi = s_hi[0][t]; ly = s_l[0][t]; hy = s_h[0][t]; }
      else prep(roi_coord(rb.start_h, rb.bin_h, ph, iy, gh), H, (W + 2) * 256, ylo, yhi, ly, hy);
      for (int ix = 0; ix < gw; ++ix) {
        int xlo, xhi; float lx, hx;
        if (fast) { const int t = pw * gw + ix; xlo = s_lo[1][t]; xhi = s_hi[1][t]; lx = s_l[1][t]; hx = s_h[1][t]; }
        else prep(roi_coord(rb.start_w, rb.bin_w, pw, ix, gw), W, 256, xlo, xhi, lx, hx);
        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
        float f1[8], f2[8], f3[8], f4[8];
        if (p.f32 == 2) {
          const long long lo2 = p.feat_lo[lvl] * 2;
          const half8 v1 = *(const half8*)(feat + (long long)(ylo + xlo) * 2), u1 = *(const half8*)(feat + lo2 + (long long)(ylo + xlo) * 2);
          const half8 v2 = *(const half8*)(feat + (long long)(ylo + xhi) * 2), u2 = *(const half8*)(feat + lo2 + (long long)(ylo + xhi) * 2);
          const half8 v3 = *(const half8*)(feat + (long long)(yhi + xlo) * 2), u3 = *(const half8*)(feat + lo2 + (long long)(yhi + xlo) * 2);
          const half8 v4 = *(const half8*)(feat + (long long)(yhi + xhi) * 2), u4 = *(const half8*)(feat + lo2 + (long long)(yhi + xhi) * 2);
#pragma unroll
          for (int c = 0; c < 8; ++c) {      // fp32(hi) + fp32(lo) is exact
            f1[c] = (float)v1[c] + (float)u1[c]; f2[c] = (float)v2[c] + (float)u2[c];
            f3[c] = (float)v3[c] + (float)u3[c]; f4[c] = (float)v4[c] + (float)u4[c];
          }
        } else if (p.f32) {
          const f32x4* q1 = (const f32x4*)(feat + (long long)(ylo + xlo) * 4);
          const f32x4* q2 = (const f32x4*)(feat + (long long)(ylo + xhi) * 4);
          const f32x4* q3 = (const f32x4*)(feat + (long long)(yhi + xlo) * 4);
          const f32x4* q4 = (const f32x4*)(feat + (long long)(yhi + xhi) * 4);
#pragma unroll
          for (int c = 0; c < 8; ++c) { f1[c] = q1[c >> 2][c & 3]; f2[c] = q2[c >> 2][c & 3]; f3[c] = q3[c >> 2][c & 3]; f4[c] = q4[c >> 2][c & 3]; }
        } else {
          const half8 v1 = *(const half8*)(feat + (long long)(ylo + xlo) * 2);
          const half8 v2 = *(const half8*)(feat + (long long)(ylo + xhi) * 2);
          const half8 v3 = *(const half8*)(feat + (long long)(yhi + xlo) * 2);
          const half8 v4 = *(const half8*)(feat + (long long)(yhi + xhi) * 2);
#pragma unroll
          for (int c = 0; c < 8; ++c) { f1[c] = (float)v1[c]; f2[c] = (float)v2[c]; f3[c] = (float)v3[c]; f4[c] = (float)v4[c]; }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float val = w1 * f1[c] + w2 * f2[c] + w3 * f3[c] + w4 * f4[c];
          acc[c] += val;
        }
      }
    }
    if (live) {
      char* op = out + (((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) * es;
      if (p.f32 == 1) {
        ((f32x4*)op)[0] = f32x4{rs_fdiv(acc[0], count), rs_fdiv(acc[1], count), rs_fdiv(acc[2], count), rs_fdiv(acc[3], count)};
        ((f32x4*)op)[1] = f32x4{rs_fdiv(acc[4], count), rs_fdiv(acc[5], count), rs_fdiv(acc[6], count), rs_fdiv(acc[7], count)};
      } else {
        half8 o, ol;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float f = rs_fdiv(acc[c], count);
          o[c] = (half_t)f;
          ol[c] = (half_t)(f - (float)o[c]);
        }
        *(half8*)op = o;
        if (p.f32 == 2) *(half8*)(op + p.out_lo * 2) = ol;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// ROIAlign, production (fp16) form.  The average over the gh x gw bilinear samples of a bin is separable:
//   out[ph][pw][c] = 1/count * sum_y sum_x  wy[ph][y] * wx[pw][x] * F[y][x][c],
// where wy[ph][y] is the sum over the bin's gh row samples of the sample's weight on feature row y (h on
// y_low, l on y_high; nothing for the samples torchvision skips) and wx likewise.  So each bin reads every cell
// of its (<= gh+2) x (<= gw+2) window ONCE instead of 4 corner cells per sample (16 -> 9 reads at g = 2,
// 64 -> 25 at g = 4): the kernel is bound by L1/L2 request rate, not HBM.  Same half-wave-per-bin, 8 channels
// per lane layout as roi_align_kernel; fp32 accumulation; the summation order differs from torchvision's
// (weights are pre-summed), which the fp32 validation mode avoids by using roi_align_kernel.
// RoIs whose window exceeds the LDS table fall back to per-sample evaluation inside this kernel.
// ---------------------------------------------------------------------------------------------
// SPLIT: the split-operand precision mode (p.f32 == 2): features and output are hi / lo fp16 planes; a cell is fp32(hi) + fp32(lo) (exact).
template <bool SPLIT>
__global__ __launch_bounds__(256, SPLIT ? 4 : 6) void roi_align_win_kernel(const RoiAlignParams p) {
  __shared__ float s_w[2][RS_ROI_PMAX][RS_ROI_WMAX];   // [0] = wy[ph][j], [1] = wx[pw][i]
  __shared__ int s_base[2][RS_ROI_PMAX], s_len[2][RS_ROI_PMAX];
  int entry = blockIdx.x;
  if (p.order) {            // XCD k (workgroups k, k+8, ...) walks the k-th eighth of the visiting order
    const int q8 = p.S >> 3, r8 = p.S & 7, x8 = entry & 7;
    entry = p.order[(x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + (entry >> 3)];
  }
  const int tid = threadIdx.x;
  int slot, n;
  const int kind = roi_entry(p, entry, slot, n);
  if (kind == 0) return;
  const int P = p.P, PP = P + 2 * p.out_pad;
  half_t* out = p.out + (long long)entry * PP * PP * 256;
  const int hw = tid >> 5, l32 = tid & 31;
  if (kind == 1) {
    half8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (half_t)0.f;
    for (int b = hw; b < P * P; b += 8) {
      const int ph = b / P, pw = b - ph * P;
      *(half8*)(out + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) = z;
      if constexpr (SPLIT) *(half8*)(out + p.out_lo + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) = z;
    }
    return;
  }
  const float* r = p.rois + (long long)slot * 4;
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const int lvl = roi_level(x1, y1, x2, y2, p.nlevels);
  if (p.out_level) { if (tid == 0) p.out_level[entry] = lvl; }
  const int H = p.H[lvl], W = p.W[lvl];
  const float sc = p.scale[lvl];
  const half_t* feat = p.feat[lvl] + ((long long)n * (H + 2) * (W + 2) + (W + 2) + 1) * 256 + l32 * 8;   // cell (0,0)
  const long long flo = SPLIT ? p.feat_lo[lvl] : 0;
  // a cell's 8 channels as floats
  auto cell = [&](const half_t* q, float (&f)[8]) {
    const half8 v = *(const half8*)q;
    if constexpr (SPLIT) {
      const half8 u = *(const half8*)(q + flo);
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = (float)v[c] + (float)u[c];
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = (float)v[c];
    }
  };
  const RoiBins rb = roi_bins(x1, y1, x2, y2, sc, P);
  const int gh = rb.gh, gw = rb.gw;
  const float count = rb.count;

  roi_tables(tid, P, rb, H, W, s_w, s_base, s_len);
  __syncthreads();
  for (int b0 = 0; b0 < P * P; b0 += 8) {
    const int b = b0 + hw;
    if (b >= P * P) break;                                  // uniform per half-wave; no barrier below
    const int ph = b / P, pw = b - ph * P;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    const int ny = s_len[0][ph], nx = s_len[1][pw];
    if (ny >= 0 && nx >= 0) {
      const half_t* f0 = feat + ((long long)s_base[0][ph] * (W + 2) + s_base[1][pw]) * 256;
      const float* wy = s_w[0][ph];
      const float* wx = s_w[1][pw];
      for (int j = 0; j < ny; ++j) {
        const float wj = wy[j];
        const half_t* fr = f0 + (long long)j * (W + 2) * 256;
        int i = 0;
        for (; i + 2 <= nx; i += 2) {
          float v0[8], v1[8];
          cell(fr + i * 256, v0);
          cell(fr + (i + 1) * 256, v1);
          const float w0 = wj * wx[i], w1 = wj * wx[i + 1];
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] += w0 * v0[c];
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] += w1 * v1[c];
        }
        if (i < nx) {
          float v0[8];
          cell(fr + i * 256, v0);
          const float w0 = wj * wx[i];
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] += w0 * v0[c];
        }
      }
    } else {
      // window larger than the table (very elongated RoI): per-sample evaluation, torchvision's order
      for (int iy = 0; iy < gh; ++iy) {
        const RoiSample sy = roi_sample(roi_coord(rb.start_h, rb.bin_h, ph, iy, gh), H);
        if (!sy.ok) continue;
        const int ylo = sy.lo, yhi = sy.hi;
        const float ly = sy.l, hy = sy.h;
        for (int ix = 0; ix < gw; ++ix) {
          const RoiSample sx = roi_sample(roi_coord(rb.start_w, rb.bin_w, pw, ix, gw), W);
          if (!sx.ok) continue;
          const int xlo = sx.lo, xhi = sx.hi;
          const float lx = sx.l, hx = sx.h;
          float v1[8], v2[8], v3[8], v4[8];
          cell(feat + ((long long)ylo * (W + 2) + xlo) * 256, v1);
          cell(feat + ((long long)ylo * (W + 2) + xhi) * 256, v2);
          cell(feat + ((long long)yhi * (W + 2) + xlo) * 256, v3);
          cell(feat + ((long long)yhi * (W + 2) + xhi) * 256, v4);
          const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[c] += w1 * v1[c] + w2 * v2[c] + w3 * v3[c] + w4 * v4[c];
        }
      }
    }
    half8 o, ol;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float f = rs_fdiv(acc[c], count);
      o[c] = (half_t)f;
      if constexpr (SPLIT) ol[c] = (half_t)(f - (float)o[c]);
    }
    *(half8*)(out + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) = o;
    if constexpr (SPLIT) *(half8*)(out + p.out_lo + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + l32 * 8) = ol;
  }
}

// ---------------------------------------------------------------------------------------------
// ROIAlign backward (training path): the adjoint of roi_align_win_kernel.  For every bin the
// incoming gradient g[ph][pw][c]/count is spread over the bin's cell window with the same separable weights,
//   dF[y][x][c] += wy[ph][y] * wx[pw][x] * g[ph][pw][c] / count,
// with float atomics into the fp32 gradient maps (as torchvision's roi_align_backward_kernel does with atomicAdd:
// [EXT tv: csrc/ops/cuda/roi_align_kernel.cu]; summation order, hence the last bits, vary from run to run there too).
// Same level assignment and per-bin tables as the forward kernel; the work is laid out per CELL of the RoI's window
// (gather over the bins that reach the cell, then one atomic per channel), see below.
// ---------------------------------------------------------------------------------------------
template <typename G>     // G: storage type of the incoming gradient (half_t, or float in the reference-precision trainer)
__global__ __launch_bounds__(256) void roi_align_bwd_kernel(const RoiAlignParams p) {
  __shared__ float s_w[2][RS_ROI_PMAX][RS_ROI_WMAX];
  __shared__ int s_base[2][RS_ROI_PMAX], s_len[2][RS_ROI_PMAX];
  __shared__ short s_lo[2][RS_ROI_CELLS], s_hi[2][RS_ROI_CELLS];
  __shared__ int s_org[2], s_ext[2];
  const int entry = blockIdx.x;
  const int tid = threadIdx.x;
  if (p.bwd_overflow && *p.bwd_overflow == 0) return;      // every entry was handled by roi_bwd_gather_kernel (the usual case)
  int slot, n;
  if (roi_entry(p, entry, slot, n) != 2) return;
  const int P = p.P, PP = P + 2 * p.out_pad;
  const G* gout = (const G*)p.out + (long long)entry * PP * PP * 256;
  const int l32 = tid & 31;
  const float* r = p.rois + (long long)slot * 4;
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const int lvl = roi_level(x1, y1, x2, y2, p.nlevels);
  const int H = p.H[lvl], W = p.W[lvl];
  const float sc = p.scale[lvl];
  float* dfeat = p.dfeat[lvl] + ((long long)n * (H + 2) * (W + 2) + (W + 2) + 1) * 256 + l32 * 8;   // cell (0,0)
  const RoiBins rb = roi_bins(x1, y1, x2, y2, sc, P);
  const int gh = rb.gh, gw = rb.gw;
  const float count = rb.count;
  roi_tables(tid, P, rb, H, W, s_w, s_base, s_len);
  __syncthreads();
  // One WAVE per bin, lane l owns channels l, l+64, l+128, l+192: every atomic instruction of the wave then covers 64
  // CONSECUTIVE floats (four full 64-byte lines) of one cell, which the L2 atomic units take as four line updates --
  // with 8 consecutive channels per lane (the forward layout) the same instruction scatters 64 words over 2 KB and the
  // kernel is ~6x slower (measured: 25.7 -> see DESIGN.md ms for 8 x 1024 RoIs).
  const int wv = tid >> 6, ln = tid & 63;
  float* dfl = dfeat - l32 * 8 + ln;              // undo the forward-style channel offset baked into dfeat

  // ---- gather form: neighbouring bins' windows overlap (by 1-2 cells on each side), so per-bin scattering issues
  // 1.5x (P=7, g=3) to 3.3x (P=14, g=2) more atomics than the RoI has cells.  Instead one wave per CELL of the RoI's whole
  // window sums the few bins that reach it (gradient tile read through L1/L2) and issues ONE atomic per channel.
  // s_lo/s_hi: per window row / column the range of bins that may cover it.
  if (tid == 0 || tid == 32) {
    const int ax = tid >> 5;
    int org, end;
    const bool bad = roi_extent(s_base[ax], s_len[ax], P, org, end);
    s_org[ax] = org;
    s_ext[ax] = bad ? -1 : end - org;
  }
  __syncthreads();
  const int eh = s_ext[0], ew = s_ext[1];
  if (eh >= 0 && ew >= 0) {
    if (p.bwd_overflow) return;                              // ... as was this one
    for (int t = tid; t < eh + ew; t += 256) {
      const int ax = t >= eh ? 1 : 0;
      const int rel = ax ? t - eh : t;
      const int y = s_org[ax] + rel;
      int lo = P, hi = 0;
      for (int b = 0; b < P; ++b) {
        const int j = y - s_base[ax][b];
        if (j >= 0 && j < s_len[ax][b] && s_w[ax][b][j] != 0.f) { lo = min(lo, b); hi = max(hi, b + 1); }
      }
      s_lo[ax][rel] = (short)lo;
      s_hi[ax][rel] = (short)hi;
    }
    __syncthreads();
    const int oy = s_org[0], ox = s_org[1];
    for (int cell = wv; cell < eh * ew; cell += 4) {           // uniform per wave; no barrier below
      const int ty = cell / ew, tx = cell - ty * ew;
      const int plo = s_lo[0][ty], phi = s_hi[0][ty], qlo = s_lo[1][tx], qhi = s_hi[1][tx];
      if (plo >= phi || qlo >= qhi) continue;
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ph = plo; ph < phi; ++ph) {
        const int jy = oy + ty - s_base[0][ph];
        if (jy < 0 || jy >= s_len[0][ph]) continue;
        const float wy = s_w[0][ph][jy];
        if (wy == 0.f) continue;
        for (int pw = qlo; pw < qhi; ++pw) {
          const int jx = ox + tx - s_base[1][pw];
          if (jx < 0 || jx >= s_len[1][pw]) continue;
          const float wgt = wy * s_w[1][pw][jx];
          if (wgt == 0.f) continue;
          const G* gp = gout + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + ln;
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] += wgt * rs_fdiv((float)gp[c * 64], count);
        }
      }
      float* d = dfl + ((long long)(oy + ty) * (W + 2) + ox + tx) * 256;
#pragma unroll
      for (int c = 0; c < 4; ++c) atomicAdd(d + c * 64, acc[c]);
    }
    return;
  }

  // ---- window larger than the tables (very elongated RoI): per-bin scatter
  for (int b0 = 0; b0 < P * P; b0 += 4) {
    const int b = b0 + wv;
    if (b >= P * P) break;                        // uniform per wave; no barrier below
    const int ph = b / P, pw = b - ph * P;
    const G* gp = gout + ((long long)(ph + p.out_pad) * PP + pw + p.out_pad) * 256 + ln;
    float gsc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) gsc[c] = rs_fdiv((float)gp[c * 64], count);
    const int ny = s_len[0][ph], nx = s_len[1][pw];
    if (ny >= 0 && nx >= 0) {
      float* f0 = dfl + ((long long)s_base[0][ph] * (W + 2) + s_base[1][pw]) * 256;
      for (int j = 0; j < ny; ++j) {
        const float wj = s_w[0][ph][j];
        if (wj == 0.f) continue;
        for (int i = 0; i < nx; ++i) {
          const float wgt = wj * s_w[1][pw][i];
          if (wgt == 0.f) continue;
          float* d = f0 + ((long long)j * (W + 2) + i) * 256;
#pragma unroll
          for (int c = 0; c < 4; ++c) atomicAdd(d + c * 64, wgt * gsc[c]);
        }
      }
    } else {
      for (int iy = 0; iy < gh; ++iy) {
        const RoiSample sy = roi_sample(roi_coord(rb.start_h, rb.bin_h, ph, iy, gh), H);
        if (!sy.ok) continue;
        const int ylo = sy.lo, yhi = sy.hi;
        const float ly = sy.l, hy = sy.h;
        for (int ix = 0; ix < gw; ++ix) {
          const RoiSample sx = roi_sample(roi_coord(rb.start_w, rb.bin_w, pw, ix, gw), W);
          if (!sx.ok) continue;
          const int xlo = sx.lo, xhi = sx.hi;
          const float lx = sx.l, hx = sx.h;
          float* d1 = dfl + ((long long)ylo * (W + 2) + xlo) * 256;
          float* d2 = dfl + ((long long)ylo * (W + 2) + xhi) * 256;
          float* d3 = dfl + ((long long)yhi * (W + 2) + xlo) * 256;
          float* d4 = dfl + ((long long)yhi * (W + 2) + xhi) * 256;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            atomicAdd(d1 + c * 64, hy * hx * gsc[c]);
            atomicAdd(d2 + c * 64, hy * lx * gsc[c]);
            atomicAdd(d3 + c * 64, ly * hx * gsc[c]);
            atomicAdd(d4 + c * 64, ly * lx * gsc[c]);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// ROIAlign backward, owner-computes form (round 3).  The atomic kernel above adds every RoI's window into the fp32 maps with one float
// atomic per cell and channel: 4 096 RoIs of ~20 x 20 cells x 256 channels are 0.4 G atomics -- 1.4 ms at batch 8, at the chip's atomic
// rate, in an order that differs from run to run (so did the weights a training run produced).  Here every 8 x 8-cell REGION of a map is
// owned by one workgroup, which walks the RoIs that reach it in ENTRY ORDER and adds their contributions into registers (64 floats per
// thread: 8 cells x 8 channels), then adds the total into the map with plain loads and stores -- no atomics, a fixed summation order,
// bit-reproducible gradients.  The per-RoI tables (the same separable weights as the forward kernel) are built once per entry by a
// pre-pass; a RoI's contribution to a cell is computed exactly as the atomic kernel computes it.  RoIs whose window exceeds the
// tables (very elongated ones) are counted and left to the atomic kernel, which otherwise returns at once.
// ---------------------------------------------------------------------------------------------
struct RoiBwdTable {
  int img, lvl;               // lvl < 0: contributes nothing (invalid slot, empty window); lvl >= 4: left to the atomic kernel
  int y0, y1, x0, x1;         // cell window [y0, y1) x [x0, x1) of the whole RoI at its level
  float count;
  int pad_;
  int base[2][RS_ROI_PMAX], len[2][RS_ROI_PMAX];
  float w[2][RS_ROI_PMAX][RS_ROI_WMAX];
};
static_assert(sizeof(RoiBwdTable) == RS_ROI_BWD_TABLE_BYTES, "RS_ROI_BWD_TABLE_BYTES");
// roi_bwd_gather_kernel stages a table from `base` on as RS_ROI_BWD_TABW raw words and reads base / len / w at these word offsets
#define RS_ROI_BWD_TABW (2 * RS_ROI_PMAX * 2 + 2 * RS_ROI_PMAX * RS_ROI_WMAX)
static_assert(sizeof(RoiBwdTable) - offsetof(RoiBwdTable, base) == RS_ROI_BWD_TABW * sizeof(int), "RS_ROI_BWD_TABW");
static_assert(offsetof(RoiBwdTable, len) - offsetof(RoiBwdTable, base) == 2 * RS_ROI_PMAX * sizeof(int), "len follows base[2][PMAX]");
static_assert(offsetof(RoiBwdTable, w) - offsetof(RoiBwdTable, base) == 4 * RS_ROI_PMAX * sizeof(int), "w follows len[2][PMAX]");

__global__ __launch_bounds__(64) void roi_bwd_prep_kernel(const RoiAlignParams p, RoiBwdTable* tabs, int* n_overflow) {
  __shared__ float s_w[2][RS_ROI_PMAX][RS_ROI_WMAX];
  __shared__ int s_base[2][RS_ROI_PMAX], s_len[2][RS_ROI_PMAX];
  const int entry = blockIdx.x, tid = threadIdx.x;
  RoiBwdTable* T = tabs + entry;
  int slot, n;
  if (roi_entry(p, entry, slot, n) != 2) { if (tid == 0) { T->img = -1; T->lvl = -1; } return; }
  const int P = p.P;
  const float* r = p.rois + (long long)slot * 4;
  const float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  const int lvl = roi_level(x1, y1, x2, y2, p.nlevels);
  const int H = p.H[lvl], W = p.W[lvl];
  const float sc = p.scale[lvl];
  const RoiBins rb = roi_bins(x1, y1, x2, y2, sc, P);
  roi_tables(tid, P, rb, H, W, s_w, s_base, s_len);               // the forward kernel's tables
  __syncthreads();
  if (tid == 0) {
    int org[2], end[2];
    bool bad = roi_extent(s_base[0], s_len[0], P, org[0], end[0]);      // the atomic kernel's own criterion for its gather form
    if (roi_extent(s_base[1], s_len[1], P, org[1], end[1])) bad = true;
    T->img = n;
    T->lvl = bad ? 4 + lvl : ((end[0] > org[0] && end[1] > org[1]) ? lvl : -1);
    T->y0 = org[0]; T->y1 = end[0]; T->x0 = org[1]; T->x1 = end[1];
    T->count = rb.count;
    if (bad) atomicAdd(n_overflow, 1);
  }
  for (int i = tid; i < 2 * RS_ROI_PMAX; i += 64) { (&T->base[0][0])[i] = (&s_base[0][0])[i]; (&T->len[0][0])[i] = (&s_len[0][0])[i]; }
  for (int i = tid; i < 2 * RS_ROI_PMAX * RS_ROI_WMAX; i += 64) (&T->w[0][0][0])[i] = (&s_w[0][0][0])[i];
}

struct RoiBwdGeom { int rh[4], rw[4], off[5]; };   // regions per level (rows, columns) and their running sum per image

template <typename G>
__device__ __forceinline__ void roi_grad8(const G* gp, float g[8]);
template <>
__device__ __forceinline__ void roi_grad8<half_t>(const half_t* gp, float g[8]) {
  const half8 v = *(const half8*)gp;
#pragma unroll
  for (int c = 0; c < 8; ++c) g[c] = (float)v[c];
}
template <>
__device__ __forceinline__ void roi_grad8<float>(const float* gp, float g[8]) {
  const f32x4 a = *(const f32x4*)gp, b = *(const f32x4*)(gp + 4);
  g[0] = a[0]; g[1] = a[1]; g[2] = a[2]; g[3] = a[3]; g[4] = b[0]; g[5] = b[1]; g[6] = b[2]; g[7] = b[3];
}

#define RS_ROI_BWD_LIST 2048     // RoIs of one image a region can meet (box head: 512 per image, mask head: 256)
template <typename G>
__global__ __launch_bounds__(256) void roi_bwd_gather_kernel(const RoiAlignParams p, const RoiBwdTable* tabs, const RoiBwdGeom geo) {
  __shared__ unsigned short s_list[RS_ROI_BWD_LIST];
  __shared__ int s_cnt, s_wave[4];
  __shared__ int s_tab[2][RS_ROI_BWD_TABW];    // two RoIs' base / len / w (the RoiBwdTable layout from `base` on): one in use, one being filled
  __shared__ float s_inv[2];
  const int tid = threadIdx.x, hw = tid >> 5, l32 = tid & 31, wv = tid >> 6, ln = tid & 63;
  const int per_image = geo.off[4];
  const int n = blockIdx.x / per_image;
  int rr = blockIdx.x - n * per_image;
  int lvl = 0;
  while (lvl < 3 && rr >= geo.off[lvl + 1]) ++lvl;
  rr -= geo.off[lvl];
  const int ry = rr / geo.rw[lvl], rx = rr - ry * geo.rw[lvl];
  const int cy0 = ry * 8, cx0 = rx * 8;
  const int H = p.H[lvl], W = p.W[lvl];
  // ---- the entries of this image that reach the region, in entry order
  int e0, e1;
  if (p.slot_list) { e0 = 0; e1 = p.S; if (p.n_entries) { const int c = *p.n_entries; e1 = c < e1 ? c : e1; } }
  else { e0 = n * p.slots_per_image; e1 = e0 + p.slots_per_image; if (e1 > p.S) e1 = p.S; }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int c0 = e0; c0 < e1; c0 += 256) {
    const int e = c0 + tid;
    bool hit = false;
    if (e < e1) {
      const RoiBwdTable* T = tabs + e;
      hit = T->lvl == lvl && T->img == n && T->y0 < cy0 + 8 && T->y1 > cy0 && T->x0 < cx0 + 8 && T->x1 > cx0;
    }
    const unsigned long long m = __ballot(hit);
    if (ln == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int pos = s_cnt + __popcll(m & ((1ull << ln) - 1ull));
    for (int w = 0; w < wv; ++w) pos += s_wave[w];
    if (hit && pos < RS_ROI_BWD_LIST) s_list[pos] = (unsigned short)(e - e0);
    __syncthreads();
    if (tid == 0) { int c = s_cnt + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]; s_cnt = c < RS_ROI_BWD_LIST ? c : RS_ROI_BWD_LIST; }
    __syncthreads();
  }
  const int cnt = s_cnt;
  if (cnt == 0) return;                         // nothing reaches the region: the map keeps what it holds
  const int P = p.P, PP = P + 2 * p.out_pad;
  const int y = cy0 + hw;                       // this half-wave's row of the region; the thread owns 8 channels of its 8 cells
  float acc[8][8];
#pragma unroll
  for (int x = 0; x < 8; ++x)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[x][c] = 0.f;
  // table of list entry k -> registers (3 words per thread), then -> s_tab[k & 1]; the loads of k + 1 are in flight under the work on k
  constexpr int TW = (RS_ROI_BWD_TABW + 255) / 256;
  int treg[TW];
  float tinv = 0.f;
  auto fetch = [&](int k) {
    const RoiBwdTable* T = tabs + e0 + s_list[k];
    const int* src = &T->base[0][0];
#pragma unroll
    for (int i = 0; i < TW; ++i) { const int o = tid + i * 256; treg[i] = o < RS_ROI_BWD_TABW ? src[o] : 0; }
    tinv = rs_fdiv(1.0f, T->count);
  };
  auto commit = [&](int k) {
#pragma unroll
    for (int i = 0; i < TW; ++i) { const int o = tid + i * 256; if (o < RS_ROI_BWD_TABW) s_tab[k & 1][o] = treg[i]; }
    if (tid == 0) s_inv[k & 1] = tinv;
  };
  fetch(0);
  commit(0);
  __syncthreads();
  for (int k = 0; k < cnt; ++k) {
    if (k + 1 < cnt) fetch(k + 1);
    const int* tb = s_tab[k & 1];
    const int* base0 = tb;                                   // [2][PMAX] base, [2][PMAX] len, [2][PMAX][WMAX] w
    const int* base1 = tb + RS_ROI_PMAX;
    const int* len0 = tb + 2 * RS_ROI_PMAX;
    const int* len1 = tb + 3 * RS_ROI_PMAX;
    const float* w0 = (const float*)(tb + 4 * RS_ROI_PMAX);
    const float* w1 = w0 + RS_ROI_PMAX * RS_ROI_WMAX;
    const float inv = s_inv[k & 1];
    // bins whose column window meets the region's 8 columns (uniform over the workgroup)
    int qlo = P, qhi = 0;
    for (int pw = 0; pw < P; ++pw)
      if (len1[pw] > 0 && base1[pw] < cx0 + 8 && base1[pw] + len1[pw] > cx0) { qlo = min(qlo, pw); qhi = max(qhi, pw + 1); }
    const G* gout = (const G*)p.out + (long long)(e0 + s_list[k]) * PP * PP * 256 + l32 * 8;
    for (int ph = 0; ph < P; ++ph) {
      const int jy = y - base0[ph];
      if (jy < 0 || jy >= len0[ph]) continue;
      const float wy = w0[ph * RS_ROI_WMAX + jy];
      if (wy == 0.f) continue;
      const float wyc = wy * inv;                            // weight of the row and 1 / (samples per bin), once per bin row
      const G* grow = gout + (long long)(ph + p.out_pad) * PP * 256;
      for (int q0 = qlo; q0 < qhi; q0 += 6) {
        float g[6][8];
#pragma unroll
        for (int u = 0; u < 6; ++u) {                        // six independent loads in flight (slots past the range re-load its first bin)
          const int pw = q0 + u < qhi ? q0 + u : qlo;
          roi_grad8<G>(grow + (long long)(pw + p.out_pad) * 256, g[u]);
        }
#pragma unroll
        for (int u = 0; u < 6; ++u) {
          const int pw = q0 + u;
          if (pw >= qhi) break;
          const int bx = base1[pw], lx = len1[pw];
          const float* wx = w1 + pw * RS_ROI_WMAX;
#pragma unroll
          for (int x = 0; x < 8; ++x) {
            const int jx = cx0 + x - bx;
            if (jx < 0 || jx >= lx) continue;
            const float wgt = wyc * wx[jx];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[x][c] += wgt * g[u][c];
          }
        }
      }
    }
    if (k + 1 < cnt) commit(k + 1);             // the other buffer was last read before the barrier that ended iteration k - 1
    __syncthreads();
  }
  if (y >= H) return;
  float* drow = p.dfeat[lvl] + (((long long)n * (H + 2) + y + 1) * (W + 2) + cx0 + 1) * 256 + l32 * 8;
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    if (cx0 + x >= W) break;
    f32x4* d = (f32x4*)(drow + (long long)x * 256);
    f32x4 a = d[0], b = d[1];
    a[0] += acc[x][0]; a[1] += acc[x][1]; a[2] += acc[x][2]; a[3] += acc[x][3];
    b[0] += acc[x][4]; b[1] += acc[x][5]; b[2] += acc[x][6]; b[3] += acc[x][7];
    d[0] = a; d[1] = b;
  }
}

}  // namespace

// ----------------------------------------------------------------------------------------------- launchers
int launch_roi_align(const RoiAlignParams& p, hipStream_t s) {
  RS_CHECK(p.C == 256, RS_ERR_UNSUPPORTED, "roi_align: C must be 256 (got %d)", p.C);
  RS_CHECK(p.S > 0, RS_ERR_ARG, "roi_align: S");
  const int use_win = rs_debug().roi_window;
  // the windowed kernel pre-sums the sample weights per feature row / column (fp32 rounding of the weights: ~1e-7 relative); the fp32 validation
  // mode keeps torchvision's per-sample order, the split-operand mode takes the window (RS_ROI_WINDOW=2: per-sample there too)
  if (!p.f32 && use_win && p.P <= RS_ROI_PMAX) hipLaunchKernelGGL(roi_align_win_kernel<false>, dim3(p.S), dim3(256), 0, s, p);
  else if (p.f32 == 2 && use_win == 1 && p.P <= RS_ROI_PMAX) hipLaunchKernelGGL(roi_align_win_kernel<true>, dim3(p.S), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(roi_align_kernel, dim3(p.S), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_roi_align_bwd(const RoiAlignParams& p_in, hipStream_t s) {
  RoiAlignParams p = p_in;
  RS_CHECK(p.C == 256 && p.P <= RS_ROI_PMAX, RS_ERR_UNSUPPORTED, "roi_align backward: C must be 256, P <= %d", RS_ROI_PMAX);
  RS_CHECK(p.S > 0, RS_ERR_ARG, "roi_align backward: S");
  for (int l = 0; l < p.nlevels; ++l) RS_CHECK(p.dfeat[l] != nullptr, RS_ERR_ARG, "roi_align backward: null gradient map");
  const bool gather = p.bwd_tables && p.bwd_overflow && p.n_images > 0 && p.nlevels == 4 && p.slots_per_image <= RS_ROI_BWD_LIST &&
                      (!p.slot_list || p.S <= RS_ROI_BWD_LIST * 8) && rs_debug().roi_bwd_atomic == 0;
  if (!gather) p.bwd_overflow = nullptr;                       // the atomic kernel serves every entry
  else {
    RoiBwdGeom geo;
    geo.off[0] = 0;
    for (int l = 0; l < 4; ++l) { geo.rh[l] = cdiv(p.H[l], 8); geo.rw[l] = cdiv(p.W[l], 8); geo.off[l + 1] = geo.off[l] + geo.rh[l] * geo.rw[l]; }
    RS_HIP(hipMemsetAsync(p.bwd_overflow, 0, sizeof(int), s));
    hipLaunchKernelGGL(roi_bwd_prep_kernel, dim3(p.S), dim3(64), 0, s, p, (RoiBwdTable*)p.bwd_tables, p.bwd_overflow);
    const dim3 grid((unsigned)(p.n_images * geo.off[4]));
    if (p.f32) hipLaunchKernelGGL(roi_bwd_gather_kernel<float>, grid, dim3(256), 0, s, p, (const RoiBwdTable*)p.bwd_tables, geo);
    else hipLaunchKernelGGL(roi_bwd_gather_kernel<half_t>, grid, dim3(256), 0, s, p, (const RoiBwdTable*)p.bwd_tables, geo);
  }
  if (p.f32) hipLaunchKernelGGL(roi_align_bwd_kernel<float>, dim3(p.S), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(roi_align_bwd_kernel<half_t>, dim3(p.S), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}
