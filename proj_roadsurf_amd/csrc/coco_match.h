// COCOeval's evaluateImg (pycocotools cocoeval.py, restated in proj_roadsurf_amd/coco_eval.py: box_iou, mask_iou_from_counts,
// _evaluate_img, match_images) as per-element rules.  Shared by coco_order_kernel / coco_match_kernel (val_ap.hip) and the host
// restatement behind rs_host_coco_match (val_ap.hip's host half); DESIGN.md section 8 ("Matching on the device") states them.
// Every translation unit that includes this header is compiled WITHOUT mul+add contraction: the float64 values must be numpy's.
//
// Scope: no crowd ground truth and no "area" override (the Python wrapper sends such a batch to the host route).
//
// TABLES, per tile, D = detection slots, K = categories, W = (D + 31) / 32, G <= gt_cap ground truths of the tile:
//   order        [D]  int32   position p -> detection slot, sorted by (category ascending, score descending, slot ascending) over the
//                             slots < count; a class outside [0, K) sorts as K, behind every category.  Positions >= count hold -1.
//   class_first  [K+1] int32  first position of each category in `order`; class_first[K] = number of detections with a category.
//   gt_per_class [K]  int32   ground truths of each category (a category has a record when this or its detections are not zero).
//   matched      [2][4][10][W] uint32   kind (0 bbox, 1 segm) x area range (all, small, medium, large) x IoU threshold; bit p % 32 of
//   ignored      [2][4][10][W] uint32   word p / 32 = the flag of position p in `order`; bits at or past class_first[K] are zero.
//   npig         [2][4][K] int32        ground truths of the category that the area range does not ignore.
// The record coco_eval.match_images gives for (category c, range a) is: the scores of order[class_first[c] .. class_first[c+1]),
// the two flag tables' bits of those positions per threshold, and npig[kind][a][c].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CM_HD __host__ __device__ __forceinline__
#else
#define CM_HD inline
#endif

#define CM_KINDS 2
#define CM_RANGES 4
#define CM_THRS 10
#define CM_MAX_SLOTS 1024      // detection slots per tile the kernels hold (order pass: classes and scores in LDS)
#define CM_MAX_GT 128          // ground truths per tile: two passes of a wave
#define CM_MAX_CLASSES 80      // = RS_MAX_CLASSES (include/rs_engine.h; ops.hip asserts it)

// coco_eval.AREA_RNG: all, small, medium, large.  32^2 lies in small and medium, 96^2 in medium and large.
CM_HD double cm_area_lo(int a) { return a == 2 ? 1024.0 : (a == 3 ? 9216.0 : 0.0); }
CM_HD double cm_area_hi(int a) { return a == 1 ? 1024.0 : (a == 2 ? 9216.0 : 1e10); }
CM_HD bool cm_out_of_range(double area, int a) { return area < cm_area_lo(a) || area > cm_area_hi(a); }

CM_HD double cm_box_area(const double b[4]) { return (b[2] - b[0]) * (b[3] - b[1]); }

// inter / union as both box_iou and mask_iou_from_counts end: np.where(union > 0, inter / np.maximum(union, 1e-300), 0.0).  The
// quotient is the compiler's float64 division: correctly rounded on the host and on gfx950.
CM_HD double cm_iou(double inter, double uni) {
  if (!(uni > 0.0)) return 0.0;
  return inter / (uni > 1e-300 ? uni : 1e-300);
}

// coco_eval.box_iou, operation for operation; d and g are XYXY
CM_HD double cm_box_iou(const double d[4], const double g[4]) {
  const double ad = cm_box_area(d), ag = cm_box_area(g);
  double w = (d[2] < g[2] ? d[2] : g[2]) - (d[0] > g[0] ? d[0] : g[0]);
  double h = (d[3] < g[3] ? d[3] : g[3]) - (d[1] > g[1] ? d[1] : g[1]);
  w = w > 0.0 ? w : 0.0;
  h = h > 0.0 ? h : 0.0;
  const double inter = w * h;
  const double uni = ad + ag - inter;
  return cm_iou(inter, uni);
}

// coco_eval.mask_iou_from_counts on one pair: the three pixel counts as float64
CM_HD double cm_mask_iou(int inter, int d_area, int g_area) {
  const double i = (double)inter;
  return cm_iou(i, (double)d_area + (double)g_area - i);
}

// the category a detection or ground truth sorts under: its own, or K for a class no category owns
CM_HD int cm_class(int cls, int K) { return cls >= 0 && cls < K ? cls : K; }

// does detection (class cj, score sj, slot j) stand before (ci, si, i)?  argsort(-scores, kind="mergesort") inside a category
CM_HD bool cm_before(int cj, float sj, int j, int ci, float si, int i) {
  if (cj != ci) return cj < ci;
  if (sj != si) return sj > si;
  return j < i;
}

// the IoU a match needs at threshold t: _evaluate_img's min(t, 1 - 1e-10)
CM_HD double cm_floor(double t) { return t < 1.0 - 1e-10 ? t : 1.0 - 1e-10; }

// A candidate of the greedy walk: rank 2 = a ground truth the range keeps, 1 = one it ignores, 0 = none.  _evaluate_img walks the kept
// ones first, then the ignored ones, each group in the tile's order, takes a candidate whose IoU is not below the best so far (so of
// equal IoUs the later one stays) and stops at the first ignored one once it holds a kept one.  That walk ends on the candidate
// that is largest under (rank, IoU, index): does b replace a?
CM_HD bool cm_replaces(int rank_b, double iou_b, int g_b, int rank_a, double iou_a, int g_a) {
  if (rank_b != rank_a) return rank_b > rank_a;
  if (iou_b != iou_a) return iou_b > iou_a;
  return g_b > g_a;
}
