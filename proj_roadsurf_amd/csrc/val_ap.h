// Validation AP on the device (val_ap.hip): ground-truth polygons rasterised onto whole canvases in the rs_dets.masks layout, and the
// pixel counts of every (detection, ground truth) pair of a batch of tiles.  DESIGN.md section 8 ("Validation AP on the device").
#pragma once
#include "common.h"
// after common.h: the HIP runtime header defines what MT_HD expands to
#include "canvas_raster.h"
#include "coco_match.h"
#include "road_vote.h"
#include "band_hist.h"

// One mask per instance, [n_inst][side][(side + 7) / 8] bytes, bit x % 8 of byte x / 8 = pixel x, padding bits zero: bit for bit
// rs_rasterize_polygons_within_box(polygons of the instance, box (0, 0, side, side), mask_size side).  Tables as MaskTargetsParams
// (polygon_pool.h).  Every byte of `out` is written, an instance without polygons gives zeros.
struct CanvasRasterParams {
  const int* inst_first;    // [n_inst + 1]
  const int* poly_off;      // [n_poly] doubles into polys
  const int* poly_len;      // [n_poly] doubles
  const double* polys;
  uint8_t* out;
  int n_inst, side;
};
int launch_canvas_raster(const CanvasRasterParams& p, hipStream_t s);

// inter [n][D][g_cap], det_area [n][D], gt_area [n][g_cap] (int32) over the detection slots < count[tile] and the ground truths
// tile_first[tile] .. tile_first[tile + 1] - 1 of gt_masks; everything else in the three tables is zero.  Masks of `bytes` bytes each
// (a multiple of 4): det_masks [n][D][bytes], gt_masks [instances][bytes].
struct PairCountParams {
  const uint8_t* det_masks;
  const int* det_count;     // [n]
  const uint8_t* gt_masks;
  const int* tile_first;    // [n + 1]
  int* inter;
  int* det_area;
  int* gt_area;
  int n, D, g_cap;
  long long bytes;
};
int launch_mask_pair_counts(const PairCountParams& p, hipStream_t s);

// COCOeval's evaluateImg for every tile of a batch, bbox and segm (coco_match.h states the rule and the layout of the five tables).
// Detections as the engine holds them ([n][D] slots, the first det_count[tile] in use); ground truths tile_first[tile] ..
// tile_first[tile + 1] - 1 of gt_boxes [instances][4] (XYXY, float64) / gt_classes [instances], at most g_cap per tile; inter /
// det_area / gt_area as PairCountParams writes them.  thrs: the ten IoU thresholds, carried by value.
struct CocoMatchParams {
  const float* det_boxes;   // [n][D][4]
  const float* det_scores;  // [n][D]
  const int* det_classes;   // [n][D]
  const int* det_count;     // [n]
  const double* gt_boxes;
  const int* gt_classes;
  const int* tile_first;    // [n + 1]
  const int* inter;         // [n][D][g_cap]
  const int* det_area;      // [n][D]
  const int* gt_area;       // [n][g_cap]
  int* order;               // [n][D]
  int* class_first;         // [n][K + 1]
  int* gt_per_class;        // [n][K]
  uint32_t* matched;        // [n][2][4][10][W]
  uint32_t* ignored;        // [n][2][4][10][W]
  int* npig;                // [n][2][4][K]
  double thrs[CM_THRS];
  int n, K, D, g_cap;
};
// both refuse (before anything is touched) null tables, K outside [1, RS_MAX_CLASSES], D outside [1, CM_MAX_SLOTS], g_cap outside
// [1, CM_MAX_GT]; `who` names the entry in the error text
int coco_match_check(const char* who, const CocoMatchParams& p);
int launch_coco_match(const CocoMatchParams& p, hipStream_t s);       // device pointers; enqueues the order pass and the match pass
int host_coco_match(const CocoMatchParams& p);                        // host pointers; the plain loops of coco_eval._evaluate_img

// The road cover vote for every tile of a batch (road_vote.h states the rule and the layout of the three tables).  Detections as the
// engine holds them; inter / gt_area as PairCountParams writes them, one "ground truth" per road label.  threshold travels by value.
struct RoadVoteParams {
  const float* det_scores;  // [n][D]
  const int* det_classes;   // [n][D]
  const int* det_count;     // [n]
  const int* tile_first;    // [n + 1]
  const int* inter;         // [n][D][g_cap]
  const int* gt_area;       // [n][g_cap]
  double* wscore;           // [n][g_cap][K]
  double* wfrac;            // [n][g_cap][K]
  int* pairs;               // [n][g_cap][K]
  double threshold;
  int n, K, D, g_cap;
};
// both refuse (before anything is touched) null tables, n < 1, K outside [1, RS_MAX_CLASSES], D or g_cap < 1, a threshold that is not
// finite (RS_ERR_ARG); D > RV_MAX_SLOTS or g_cap > RV_MAX_GT (RS_ERR_UNSUPPORTED); `who` names the entry in the error text
int road_vote_check(const char* who, const RoadVoteParams& p);
int launch_road_votes(const RoadVoteParams& p, hipStream_t s);        // device pointers; clears the three tables and enqueues the kernel
int host_road_votes(const RoadVoteParams& p);                         // host pointers; the plain loops

// The same for a list of thresholds at once (road_vote.h, THE SWEEP): slice j of the three tables has the bits of RoadVoteParams'
// tables at thresholds[j].  The list travels by value; entries at and past T are not read.
struct RoadVoteSweepParams {
  const float* det_scores;  // [n][D]
  const int* det_classes;   // [n][D]
  const int* det_count;     // [n]
  const int* tile_first;    // [n + 1]
  const int* inter;         // [n][D][g_cap]
  const int* gt_area;       // [n][g_cap]
  double* wscore;           // [n][T][g_cap][K]
  double* wfrac;            // [n][T][g_cap][K]
  int* pairs;               // [n][T][g_cap][K]
  double thresholds[RV_SWEEP_MAX];
  int T;
  int n, K, D, g_cap;
};
// both refuse (before anything is touched) what road_vote_check refuses, T outside [1, RV_SWEEP_MAX] and an entry below T that is
// not finite (RS_ERR_ARG); `who` names the entry in the error text
int road_vote_sweep_check(const char* who, const RoadVoteSweepParams& p);
int launch_road_votes_sweep(const RoadVoteSweepParams& p, hipStream_t s);   // device pointers; clears the three tables and enqueues the kernel
int host_road_votes_sweep(const RoadVoteSweepParams& p);                    // host pointers; the plain loops

// The band histograms of the road labels of a batch of tiles (band_hist.h states the rule and the layout).  tiles as the engine holds
// them, label_masks as CanvasRasterParams writes them, one canvas per label instance.
struct BandHistParams {
  const uint8_t* tiles;        // [n][side][side][C]
  const uint8_t* label_masks;  // [n_inst][side][(side + 7) / 8]
  const int* tile_first;       // [n + 1]
  uint32_t* hist;              // [n_inst][C][256]
  int n, n_inst, side, C;
};
// both refuse (before anything is touched) a null table, n < 1, n_inst < 0, side outside [1, BH_MAX_SIDE], C outside [1,
// BH_MAX_CHANNELS] (RS_ERR_ARG); canvases that are not whole 32-bit words (RS_ERR_UNSUPPORTED); `who` names the entry in the error text
int band_hist_check(const char* who, const BandHistParams& p);
int launch_band_hist(const BandHistParams& p, hipStream_t s);         // device pointers; clears hist and enqueues the kernel
int host_band_hist(const BandHistParams& p);                          // host pointers; the plain loops
