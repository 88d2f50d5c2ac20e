// The road cover vote on polygon areas (poly_vote.hip): the overlap of every (road label, detection) pair of a batch of tiles on the
// polygoniser's vertex tables and the labels' float64 rings (poly_overlap.h states the rule), and the vote's walk on those weights
// (road_vote.h, rv_pair_area).  DESIGN.md section 3.5 ("polygon geometry").
#pragma once
#include "common.h"
// after common.h: the HIP runtime header defines what PO_HD / RV_HD expand to
#include "poly_overlap.h"
#include "road_vote.h"

// Detections: the polygoniser's tables over n * D instances (instance = tile * D + slot; header offsets into the three shared tables),
// the first det_count[tile] slots of a tile in use.  Labels: the packed pool of polygon_pool.h -- tile_first [n + 1] (first label of
// every tile), inst_first [labels + 1] (first ring of every label), poly_off [rings] (doubles into polys), poly_len [rings] (doubles),
// polys float64 tile pixels.  Out: frac [n][D][g_cap] and label_area [n][g_cap] double, flagged [n] int32 = the tile's flagged
// instances among its slots in use (their pairs are 0: the caller redoes that batch); everything outside the tiles' own labels and
// slots in use is zero.
struct PolyOverlapParams {
  const int* header;           // [n * D][PO_HDR]
  const int* poly_ring_count;
  const int* ring_len;
  const int16_t* xy;
  const int* det_count;        // [n]
  const int* tile_first;       // [n + 1]
  const int* inst_first;
  const int* poly_off;
  const int* poly_len;
  const double* polys;
  double* frac;                // [n][D][g_cap]
  double* label_area;          // [n][g_cap]
  int* flagged;                // [n]
  int n, D, g_cap;
  int raw_areas;               // != 0: the last step is left out and `frac` holds the areas themselves (tests, diagnostics)
};
// both refuse (before anything is touched) a null table, n < 1, D or g_cap < 1 (RS_ERR_ARG); D > RV_MAX_SLOTS or g_cap > RV_MAX_GT
// (RS_ERR_UNSUPPORTED), as road_vote_check; `who` names the entry in the error text
int poly_overlap_check(const char* who, const PolyOverlapParams& p);
int launch_poly_overlaps(const PolyOverlapParams& p, hipStream_t s);   // device pointers; clears the three tables and enqueues the kernel
int host_poly_overlaps(const PolyOverlapParams& p);                    // host pointers; the plain loops in the kernel's summation order

// The vote's sweep (road_vote.h, THE SWEEP) reading frac in place of rv_frac(inter, area): slice j of the three tables is the walk of
// rv_pair_area at thresholds[j]; the single vote is T = 1.  The list travels by value; entries at and past T are not read.
struct RoadVoteAreaSweepParams {
  const float* det_scores;  // [n][D]
  const int* det_classes;   // [n][D]
  const int* det_count;     // [n]
  const int* tile_first;    // [n + 1]
  const double* frac;       // [n][D][g_cap]
  double* wscore;           // [n][T][g_cap][K]
  double* wfrac;            // [n][T][g_cap][K]
  int* pairs;               // [n][T][g_cap][K]
  double thresholds[RV_SWEEP_MAX];
  int T;
  int n, K, D, g_cap;
};
// both refuse (before anything is touched) what road_vote_sweep_check refuses, with the same codes
int road_vote_area_sweep_check(const char* who, const RoadVoteAreaSweepParams& p);
int launch_road_votes_area_sweep(const RoadVoteAreaSweepParams& p, hipStream_t s);   // device pointers; clears the tables and enqueues the kernel
int host_road_votes_area_sweep(const RoadVoteAreaSweepParams& p);                    // host pointers; the plain loops
