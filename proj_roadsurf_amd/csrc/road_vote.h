// The road cover vote (R:scripts/road_segmentation/determine_class.py:97-190, restated in proj_roadsurf_amd/raster_vote.py:
// weighted_scores, determine_detected_class) on pixel counts, as a per-cell rule.  Shared by road_vote_kernel (val_ap.hip) and the
// host restatement behind rs_host_road_votes (val_ap.hip's host half); DESIGN.md section 3.5 states it.
// Every translation unit that includes this header is compiled WITHOUT mul+add contraction: the float64 values must be numpy's.
//
// A cell is (tile t, label g, class c).  Its detections are the slots d = 0 .. det_count[t] - 1 in ascending order; the pair (g, d)
// votes in the cell when
//   I = inter[t][d][g] > 0,  det_classes[t][d] == c,
//   frac = rint((double)I / (double)A * 100.0) / 100.0 > 0.05      (A = gt_area[t][g] > 0; np.round(I / A, 2)),
//   (double)score >= threshold                                     (determine_detected_class's `threshold`),
// and then adds  ws += frac * (double)score,  wa += frac,  pairs += 1,  each accumulator starting at zero.  The quotient is the
// compiler's float64 division: correctly rounded on the host and on gfx950.  rint rounds half to even, as np.round.
//
// TABLES, per tile, K = classes: wscore [gt_cap][K] double, wfrac [gt_cap][K] double, pairs [gt_cap][K] int32.  Rows of labels at or
// past the tile's own (tile_first[t + 1] - tile_first[t], at most gt_cap) and rows of labels with area 0 are zero; a detection whose
// class lies outside [0, K) votes for nothing.  One cell has one owner and a fixed order: two runs give the same bits.
//
// THE SWEEP (R:scripts/road_segmentation/final_metrics.py runs determine_detected_class once per score threshold): a list
// thresholds[0 .. T - 1], 1 <= T <= RV_SWEEP_MAX, any finite doubles in any order, duplicates allowed.  Entry j of every cell is what
// the walk above accumulates with threshold = thresholds[j] -- rv_pair itself, slot for slot, so slice j of the sweep's tables
// (wscore, wfrac [T][gt_cap][K] double and pairs [T][gt_cap][K] int32 per tile) has the bits of the single-threshold tables at
// thresholds[j].  road_vote_sweep_kernel walks the slots once per (cell, threshold) with the threshold as one value for the wave.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RV_HD __host__ __device__ __forceinline__
#else
#define RV_HD inline
#endif

#define RV_MAX_SLOTS 1024      // detection slots per tile (= CM_MAX_SLOTS, the capacity of the tables in front of this stage)
#define RV_MAX_GT 128          // labels per tile (= RS_EVAL_GT_CAP)
#define RV_MAX_CLASSES 80      // = RS_MAX_CLASSES
#define RV_SWEEP_MAX 32        // thresholds per sweep (= RS_VOTE_SWEEP_MAX)

struct RvCell {
  double ws, wa;
  int pairs;
};

RV_HD void rv_clear(RvCell* a) { a->ws = 0.0; a->wa = 0.0; a->pairs = 0; }

// np.round(I / A, 2) of two pixel counts, A > 0
RV_HD double rv_frac(int inter, int area) {
  const double q = (double)inter / (double)area;
  const double m = rint(q * 100.0);
  return m / 100.0;
}

// one detection slot of the walk of cell (label of area `area` > 0, class c)
RV_HD void rv_pair(RvCell* a, int inter, int area, int cls, float score, int c, double threshold) {
  if (inter <= 0 || cls != c) return;
  const double frac = rv_frac(inter, area);
  const double s = (double)score;
  if (!(frac > 0.05) || !(s >= threshold)) return;
  a->ws += frac * s;
  a->wa += frac;
  a->pairs += 1;
}

// The same slot of the walk on POLYGON areas (poly_overlap.h): frac arrives rounded (po_frac: np.round(area(label ∩ detection) /
// area(label), 2), 0 for a pair without overlap), so the count test and the division of rv_pair fall away and the rest is its text.
RV_HD void rv_pair_area(RvCell* a, double frac, int cls, float score, int c, double threshold) {
  if (cls != c) return;
  const double s = (double)score;
  if (!(frac > 0.05) || !(s >= threshold)) return;
  a->ws += frac * s;
  a->wa += frac;
  a->pairs += 1;
}

// the labels of tile t that the stage reads, and its detections: clamped to the tables' capacities
RV_HD int rv_tile_labels(const int* tile_first, int t, int gt_cap) {
  const int G = tile_first[t + 1] - tile_first[t];
  return G > gt_cap ? gt_cap : (G < 0 ? 0 : G);
}
RV_HD int rv_tile_dets(const int* det_count, int t, int slots) {
  const int c = det_count[t];
  return c > slots ? slots : (c < 0 ? 0 : c);
}
