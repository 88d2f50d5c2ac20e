// Sampling geometry of ROIPooler + ROIAlign(aligned = true, sampling_ratio = 0), stated once: which FPN level a box goes to, its bins
// and samples per bin, what one sample coordinate reads, and the separable per-bin weight tables built from those.  Nothing here
// touches features.  The five RoIAlign kernels (roi_align.hip) and rpn_merge_kernel's visiting order (detect_kernels.hip) share it:
// the backward is the adjoint of the forward, and the owner-computes backward equals the atomic one, because they call the same
// functions.  The header also compiles for the host (tests/test_roi_geom_cpu.py); there a division is the plain `/`, which common.h
// documents rs_fdiv to be bit-identical to.  All arithmetic is fp32 in torchvision's / detectron2's operation order: compile without
// mul+add contraction, and keep every expression as it is -- several sit next to a rounding tie (see fpn_level).
// [EXT d2: modeling/poolers.py; EXT tv: csrc/ops/cuda/roi_align_kernel.cu]
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "common.h"
#define RG_D __device__ __forceinline__
RG_D float rg_div(float a, float b) { return rs_fdiv(a, b); }
#else
#include <math.h>
#define RG_D inline
RG_D float rg_div(float a, float b) { return a / b; }
#endif

#define RS_ROI_MAXS 512    // roi_align_kernel: sample coordinates per axis held in LDS (P * g)
#define RS_ROI_WMAX 24     // window rows/cols per bin held in the weight tables (g <= 22)
#define RS_ROI_PMAX 14
#define RS_ROI_CELLS 320   // rows/cols of a whole RoI window the gather forms of the backward handle (14 bins x 22 samples + 2 at most)

RG_D float rg_f32(uint32_t bits) { float f; __builtin_memcpy(&f, &bits, sizeof f); return f; }

// assign_boxes_to_levels [EXT d2: modeling/poolers.py]: floor(4 + log2(v)) clamped to [2,5], minus 2, where
// v = sqrt(area) / 224 + 1e-8 (fp32) and the log2 and the add are fp32 too.  The level is monotone in v, so it is decided by
// three fp32 cut points: the smallest v of levels 1, 2, 3.  They are NOT 0.5, 1, 2: for v a few ulps below each power of two,
// log2(v) rounds to within half an ulp of the integer, and 4 + log2(v) rounds up onto it.  The cut points below are those of a
// correctly rounded log2 (tests/test_oracle_kat.py re-derives them); a device log2f is not used, since at 0.49999994 and
// 0.49999997 the fp32 sum lies on or next to a rounding tie and a 1-ulp log2 error changes the level.
RG_D int fpn_level(float v) {
  const float c1 = rg_f32(0x3efffffeu);   // 0.49999994
  const float c2 = rg_f32(0x3f7fffffu);   // 0.99999994
  const float c3 = rg_f32(0x3ffffffdu);   // 1.9999996
  return v >= c3 ? 3 : (v >= c2 ? 2 : (v >= c1 ? 1 : 0));
}

// box -> index of its FPN level among the `nlevels` maps from p2 up
RG_D int roi_level(float x1, float y1, float x2, float y2, int nlevels) {
  const float area = (x2 - x1) * (y2 - y1);
  const float v = rg_div(sqrtf(area), 224.0f) + 1e-8f;
  int lvl = fpn_level(v);
  if (lvl > nlevels - 1) lvl = nlevels - 1;
  return lvl;
}

// entry -> slot -> image.  0: past the entries (nothing is read or written for it); 1: an empty slot of its image (the forward writes
// zeros, the backward nothing); 2: a RoI to pool.  Prm: RoiAlignParams, or whatever has its S / n_entries / slot_list / slots_per_image /
// per_image_count.
template <class Prm>
RG_D int roi_entry(const Prm& p, int entry, int& slot, int& n) {
  int n_entries = p.S;
  if (p.n_entries) { const int c = *p.n_entries; n_entries = c < n_entries ? c : n_entries; }
  if (entry >= n_entries) return 0;
  slot = p.slot_list ? p.slot_list[entry] : entry;
  n = slot / p.slots_per_image;
  if (p.per_image_count && (slot - n * p.slots_per_image) >= p.per_image_count[n]) return 1;
  return 2;
}

// A box on a map of scale sc, pooled to P x P bins: origin, bin size, samples per bin (adaptive) and their number as the divisor.
struct RoiBins {
  float start_w, start_h, bin_w, bin_h;
  int gh, gw;
  float count;
};
RG_D RoiBins roi_bins(float x1, float y1, float x2, float y2, float sc, int P) {
  RoiBins r;
  r.start_w = x1 * sc - 0.5f;
  r.start_h = y1 * sc - 0.5f;
  const float roi_w = (x2 * sc - 0.5f) - r.start_w;
  const float roi_h = (y2 * sc - 0.5f) - r.start_h;
  r.bin_h = rg_div(roi_h, (float)P);
  r.bin_w = rg_div(roi_w, (float)P);
  r.gh = (int)ceilf(rg_div(roi_h, (float)P));
  r.gw = (int)ceilf(rg_div(roi_w, (float)P));
  if (r.gh < 0) r.gh = 0;
  if (r.gw < 0) r.gw = 0;
  r.count = (float)((r.gh * r.gw) > 1 ? (r.gh * r.gw) : 1);
  return r;
}

// coordinate of sample i (of g) of bin b along one axis
RG_D float roi_coord(float start, float bin, int b, int i, int g) {
  return start + (float)b * bin + rg_div(((float)i + 0.5f) * bin, (float)g);
}

// One sample coordinate on an axis of `size` cells -> the two cells it reads and their weights (h on lo, l on hi).  ok == false:
// torchvision skips the sample (it contributes 0); the rest is zero then, which is roi_align_kernel's zero-weight form.
// Returned by value: with reference outputs that a skipped sample leaves unwritten the compiler carried them round the sample
// loops as live values (roi_align_win_kernel<false> spilled 69 VGPRs instead of 13, roi_align_bwd_kernel lost a wave of occupancy).
struct RoiSample {
  int lo, hi;
  float l, h;
  bool ok;
};
RG_D RoiSample roi_sample(float c, int size) {
  RoiSample s = {0, 0, 0.f, 0.f, !(c < -1.0f || c > (float)size)};
  if (!s.ok) return s;
  if (c <= 0.f) c = 0.f;
  s.lo = (int)c;
  if (s.lo >= size - 1) { s.hi = s.lo = size - 1; c = (float)s.lo; } else { s.hi = s.lo + 1; }
  s.l = c - (float)s.lo;
  s.h = 1.f - s.l;
  return s;
}

// Separable weight table of bin b along one axis: w[j] = the summed weight of the bin's g samples on cell base + j, j < len
// (serial over the samples, in sample order, so the pre-summed weights are deterministic).  len = -1: the bin's window does not fit
// RS_ROI_WMAX cells (a very elongated RoI), the caller evaluates per sample.
RG_D void roi_axis_table(float start, float bin, int b, int g, int size, float* w, int& base_out, int& len_out) {
  for (int j = 0; j < RS_ROI_WMAX; ++j) w[j] = 0.f;
  int base = 0, len = 0;
  bool have = false, overflow = false;
  for (int i = 0; i < g; ++i) {
    const RoiSample s = roi_sample(roi_coord(start, bin, b, i, g), size);
    if (!s.ok) continue;
    if (!have) { base = s.lo; have = true; }
    if (s.hi - base >= RS_ROI_WMAX) { overflow = true; break; }
    w[s.lo - base] += s.h;
    w[s.hi - base] += s.l;
    len = s.hi - base + 1;
  }
  base_out = base;
  len_out = overflow ? -1 : len;
}

// Both axes' tables of a RoI, [0] = rows (wy[ph][j]), [1] = columns (wx[pw][i]): threads 0..P-1 build the row tables, 32..32+P-1 the
// column tables; the caller synchronises.
RG_D void roi_tables(int tid, int P, const RoiBins& r, int H, int W, float (*s_w)[RS_ROI_PMAX][RS_ROI_WMAX], int (*s_base)[RS_ROI_PMAX],
                     int (*s_len)[RS_ROI_PMAX]) {
  if ((tid < P) || (tid >= 32 && tid < 32 + P)) {
    const int ax = tid >= 32 ? 1 : 0;
    const int b = ax ? tid - 32 : tid;
    roi_axis_table(ax ? r.start_w : r.start_h, ax ? r.bin_w : r.bin_h, b, ax ? r.gw : r.gh, ax ? W : H, s_w[ax][b], s_base[ax][b], s_len[ax][b]);
  }
}

// Cell range [org, end) of the whole RoI along one axis from its P bins' tables.  true ("bad"): a bin overflowed its table or the
// range exceeds RS_ROI_CELLS -- the RoI is left to the per-bin scatter of roi_align_bwd_kernel.
RG_D bool roi_extent(const int* base, const int* len, int P, int& org_out, int& end_out) {
  int org = 0x7fffffff, end = -1;
  bool bad = false;
  for (int b = 0; b < P; ++b) {
    if (len[b] < 0) { bad = true; break; }
    if (len[b] == 0) continue;
    org = org < base[b] ? org : base[b];
    end = end > base[b] + len[b] ? end : base[b] + len[b];
  }
  if (end < 0) { org = 0; end = 0; }
  if (end - org > RS_ROI_CELLS) bad = true;
  org_out = org;
  end_out = end;
  return bad;
}
