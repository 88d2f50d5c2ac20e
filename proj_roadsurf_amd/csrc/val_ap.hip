// Validation AP on the device: the two kernels between the engine's bit-packed detection masks and the integer
// tables coco_eval.match_images takes for `segm`, and the two that run match_images' own step (COCOeval's evaluateImg) behind them.
//   canvas_raster_kernel      ground-truth polygons -> bit-packed canvases, bit for bit the host's rs_rasterize_polygons_within_box at
//                             box (0, 0, side, side): the per-column closed form of canvas_raster.h, fp64 in the host's operand order
//                             (compiled without mul+add contraction), integer LDS atomics only.
//   mask_pair_counts_kernel   popcounts of detection AND ground truth for every pair of every tile of a batch, with both sides' own
//                             areas.  Integers only.
//   coco_order_kernel         per tile the detections' order by (category, score descending, slot) and the per-category counts.
//   coco_match_kernel         one wave per (tile, kind, area range, IoU threshold): the greedy matching over coco_match.h's rules, float64
//                             IoUs with the compiler's correctly rounded division, flags as bit words.  No atomics.
//   road_vote_kernel          the road cover vote (road_vote.h) on the same pair counts, one road label per "ground truth": one work
//                             item per (label, class) cell, float64 in numpy's order.  No atomics.
//   road_vote_sweep_kernel    the same walk for a list of score thresholds, the threshold's index in blockIdx.z: slice j of its tables has
//                             the bits of road_vote_kernel's at thresholds[j].
// host_coco_match, host_road_votes and host_road_votes_sweep are the same rules as plain host loops (rs_host_coco_match,
// rs_host_road_votes, rs_host_road_votes_sweep); they live here for the compile flags.
#include <string.h>

#include "val_ap.h"

namespace {

constexpr int CR_STRIP = 32;                       // columns per workgroup = one 32-bit word of every output row
constexpr int CR_WORDS = CR_MAX_SIDE / 32;         // 32-bit words of one column's rows

// One workgroup per (strip of 32 columns, instance).  Per polygon: every lane takes edges, walks the columns of the strip that the
// edge's x-range reaches and toggles the bit of the row its point lands on; a prefix parity down each column turns the points into
// the fill; the polygons of the instance are ORed.  Then the strip is transposed: one lane per row gathers its 32 column bits into
// the row's word.  Every loop bound is known before the loop.
__global__ __launch_bounds__(256) void canvas_raster_kernel(const CanvasRasterParams p) {
  __shared__ uint32_t s_pts[CR_STRIP][CR_WORDS];
  __shared__ uint32_t s_acc[CR_STRIP][CR_WORDS];
  const int S = p.side, W = (S + 31) >> 5, inst = blockIdx.y, tid = threadIdx.x;
  const int lo = blockIdx.x * CR_STRIP, hi = lo + CR_STRIP - 1 < S - 1 ? lo + CR_STRIP - 1 : S - 1;
  const int cells = CR_STRIP * W;
  for (int i = tid; i < cells; i += 256) s_acc[i / W][i % W] = 0;
  const MtBox box = mt_box(0.f, 0.f, (float)S, (float)S, S);       // ratio S / S = 1: the host's call with box (0, 0, side, side)
  const int q0 = p.inst_first[inst], q1 = p.inst_first[inst + 1];
  for (int q = q0; q < q1; ++q) {
    for (int i = tid; i < cells; i += 256) s_pts[i / W][i % W] = 0;
    __syncthreads();
    const double* xy = p.polys + p.poly_off[q];
    const int k = p.poly_len[q] >> 1;
    for (int j = tid; j < k; j += 256) {
      const int j2 = j + 1 == k ? 0 : j + 1;
      int xs, ys, xe, ye, m0, m1;
      mt_vertex(box, xy[2 * j], xy[2 * j + 1], &xs, &ys);
      mt_vertex(box, xy[2 * j2], xy[2 * j2 + 1], &xe, &ye);
      cr_edge_columns(xs, xe, lo, hi, &m0, &m1);
      for (int m = m0; m <= m1; ++m) {
        const int r = cr_edge_row(xs, ys, xe, ye, m, S);
        if (r >= 0) atomicXor(&s_pts[m - lo][r >> 5], 1u << (r & 31));
      }
    }
    __syncthreads();
    for (int i = tid; i < cells; i += 256) {      // (column, word) i keeps its lane from polygon to polygon: s_acc needs no atomics
      const int mi = i / W, w = i - mi * W;
      uint32_t carry = 0;
      for (int u = 0; u < w; ++u) carry ^= (uint32_t)__popc(s_pts[mi][u]);
      s_acc[mi][w] |= cr_prefix_parity(s_pts[mi][w], carry & 1u);
    }
    __syncthreads();                              // the points are cleared again for the next polygon
  }
  __syncthreads();
  const int Wb = (S + 7) >> 3, nb = Wb - 4 * (int)blockIdx.x < 4 ? Wb - 4 * (int)blockIdx.x : 4;
  for (int y = tid; y < S; y += 256) {
    uint32_t row = 0;                             // columns past `hi` never received a point: the padding bits are zero
    for (int mi = 0; mi < CR_STRIP; ++mi) row |= ((s_acc[mi][y >> 5] >> (y & 31)) & 1u) << mi;
    uint8_t* o = p.out + ((long long)inst * S + y) * Wb + 4 * blockIdx.x;
    if (nb == 4 && (Wb & 3) == 0) *(uint32_t*)o = row;              // rows of whole words: every mask starts on a word
    else for (int b = 0; b < nb; ++b) o[b] = (uint8_t)(row >> (8 * b));
  }
}

constexpr int PC_CHUNK = 8192;                     // words of a detection mask held in LDS at a time (32 KB)

// One workgroup per (detection slot, tile), plus one per tile (blockIdx.x == D) for the areas of the tile's ground truths.  The
// detection mask is staged in LDS chunk by chunk (read once, its area counted on the way) and the tile's ground truths are streamed
// against it, one wave per ground truth.
__global__ __launch_bounds__(256) void mask_pair_counts_kernel(const PairCountParams p) {
  __shared__ uint32_t s_det[PC_CHUNK];
  __shared__ int s_red[4];
  const int t = blockIdx.y, d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = (int)(p.bytes >> 2);
  const int g0 = p.tile_first[t];
  int G = p.tile_first[t + 1] - g0;
  G = G > p.g_cap ? p.g_cap : (G < 0 ? 0 : G);
  const uint32_t* GT = (const uint32_t*)p.gt_masks + (long long)g0 * words;
  if (d == p.D) {
    for (int g = wave; g < G; g += 4) {
      const uint32_t* L = GT + (long long)g * words;
      int c = 0;
      for (int i = lane; i < words; i += 64) c += __popc(L[i]);
      for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
      if (lane == 0) p.gt_area[(long long)t * p.g_cap + g] = c;
    }
    return;
  }
  if (d >= p.det_count[t]) return;                // uniform per workgroup; the tables were zeroed by the launcher
  const uint32_t* Dm = (const uint32_t*)p.det_masks + ((long long)t * p.D + d) * words;
  int* row = p.inter + ((long long)t * p.D + d) * p.g_cap;
  int area = 0;
  for (int base = 0; base < words; base += PC_CHUNK) {
    const int nw = words - base < PC_CHUNK ? words - base : PC_CHUNK;
    __syncthreads();                              // the previous chunk has been read
    for (int i = tid; i < nw; i += 256) {
      const uint32_t v = Dm[base + i];
      s_det[i] = v;
      area += __popc(v);
    }
    __syncthreads();
    for (int g = wave; g < G; g += 4) {
      const uint32_t* L = GT + (long long)g * words + base;
      int c = 0;
      for (int i = lane; i < nw; i += 64) c += __popc(s_det[i] & L[i]);
      for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
      if (lane == 0) row[g] = (base ? row[g] : 0) + c;              // pair (d, g) belongs to this lane alone
    }
  }
  for (int off = 32; off > 0; off >>= 1) area += __shfl_down(area, off);
  if (lane == 0) s_red[wave] = area;
  __syncthreads();
  if (tid == 0) p.det_area[(long long)t * p.D + d] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// ---- COCOeval's evaluateImg (coco_match.h) ----

// the ground truths of tile t that the kernels read: their first instance and their number, clamped to the capacity
__device__ __forceinline__ int cm_tile_gts(const CocoMatchParams& p, int t, int* g0) {
  *g0 = p.tile_first[t];
  const int G = p.tile_first[t + 1] - *g0;
  return G > p.g_cap ? p.g_cap : (G < 0 ? 0 : G);
}
__device__ __forceinline__ int cm_tile_dets(const CocoMatchParams& p, int t) {
  const int c = p.det_count[t];
  return c > p.D ? p.D : (c < 0 ? 0 : c);
}
// the area the range is checked against: bbox = the box's own in float64, segm = the pixel count
__device__ __forceinline__ double cm_gt_area(const CocoMatchParams& p, int kind, int t, int g0, int g) {
  return kind ? (double)p.gt_area[(long long)t * p.g_cap + g] : cm_box_area(p.gt_boxes + 4ll * (g0 + g));
}

// Order pass, one workgroup per tile: the rank of every detection by counting those that stand before it (cm_before), the first
// position of every category, the ground truths per category and those each range keeps.  Every loop runs to a clamped count.
__global__ __launch_bounds__(256) void coco_order_kernel(const CocoMatchParams p) {
  __shared__ int s_cls[CM_MAX_SLOTS];
  __shared__ float s_score[CM_MAX_SLOTS];
  __shared__ int s_order[CM_MAX_SLOTS];
  const int t = blockIdx.x, tid = threadIdx.x, K = p.K, D = p.D;
  const int n = cm_tile_dets(p, t);
  int g0;
  const int G = cm_tile_gts(p, t, &g0);
  for (int i = tid; i < D; i += 256) {
    s_order[i] = -1;
    if (i < n) {
      s_cls[i] = cm_class(p.det_classes[(long long)t * D + i], K);
      s_score[i] = p.det_scores[(long long)t * D + i];
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const int ci = s_cls[i];
    const float si = s_score[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += cm_before(s_cls[j], s_score[j], j, ci, si, i);
    s_order[rank] = i;                            // rank < n; scores that are not ordered (NaN) may share one, the others stay -1
  }
  for (int c = tid; c <= K; c += 256) {
    int first = 0;
    for (int j = 0; j < n; ++j) first += s_cls[j] < c;
    p.class_first[(long long)t * (K + 1) + c] = first;
  }
  for (int c = tid; c < K; c += 256) {
    int k = 0;
    for (int g = 0; g < G; ++g) k += p.gt_classes[g0 + g] == c;
    p.gt_per_class[(long long)t * K + c] = k;
  }
  for (int i = tid; i < CM_KINDS * CM_RANGES * K; i += 256) {
    const int c = i % K, a = (i / K) % CM_RANGES, kind = i / (K * CM_RANGES);
    int k = 0;
    for (int g = 0; g < G; ++g) k += p.gt_classes[g0 + g] == c && !cm_out_of_range(cm_gt_area(p, kind, t, g0, g), a);
    p.npig[(long long)t * CM_KINDS * CM_RANGES * K + i] = k;
  }
  __syncthreads();
  for (int i = tid; i < D; i += 256) p.order[(long long)t * D + i] = s_order[i];
}

// Match pass, one wave per (tile, kind, area range, threshold).  The detections are walked in `order`; lane l holds ground truths l
// and l + 64 of the tile (class, ignore flag, matched flag, box) in registers, computes its candidates' IoUs against the detection and
// the wave reduces them to the one cm_replaces ranks highest.  The flags collect in LDS, one bit per position.
__global__ __launch_bounds__(64) void coco_match_kernel(const CocoMatchParams p) {
  __shared__ uint32_t s_m[CM_MAX_SLOTS / 32];
  __shared__ uint32_t s_i[CM_MAX_SLOTS / 32];
  const int t = blockIdx.y, lane = threadIdx.x, K = p.K, D = p.D, W = (D + 31) >> 5;
  const int ti = blockIdx.x % CM_THRS, a = (blockIdx.x / CM_THRS) % CM_RANGES, kind = blockIdx.x / (CM_THRS * CM_RANGES);
  const double need = cm_floor(p.thrs[ti]);
  const int n = cm_tile_dets(p, t);
  int g0;
  const int G = cm_tile_gts(p, t, &g0);
  for (int w = lane; w < W; w += 64) s_m[w] = s_i[w] = 0;
  int gcls[2], grank[2];                          // grank: 2 = kept by the range, 1 = ignored, 0 = no such ground truth or matched
  double gbox[2][4];
  int garea[2];
  for (int q = 0; q < 2; ++q) {
    const int g = lane + 64 * q;
    gcls[q] = -1; grank[q] = 0; garea[q] = 0;
    gbox[q][0] = gbox[q][1] = gbox[q][2] = gbox[q][3] = 0.0;
    if (g < G) {
      gcls[q] = p.gt_classes[g0 + g];
      grank[q] = cm_out_of_range(cm_gt_area(p, kind, t, g0, g), a) ? 1 : 2;
      if (kind) garea[q] = p.gt_area[(long long)t * p.g_cap + g];
      else for (int k = 0; k < 4; ++k) gbox[q][k] = p.gt_boxes[4ll * (g0 + g) + k];
    }
  }
  __syncthreads();
  for (int pos = 0; pos < n; ++pos) {
    const int slot = p.order[(long long)t * D + pos];                // uniform
    if (slot < 0 || slot >= D) continue;
    const int c = p.det_classes[(long long)t * D + slot];
    if (c < 0 || c >= K) continue;
    double db[4];
    for (int k = 0; k < 4; ++k) db[k] = (double)p.det_boxes[((long long)t * D + slot) * 4 + k];
    const int darea = kind ? p.det_area[(long long)t * D + slot] : 0;
    const int* irow = p.inter + ((long long)t * D + slot) * p.g_cap;
    int rank = 0, who = -1;
    double iou = 0.0;
    for (int q = 0; q < 2; ++q) {
      const int g = lane + 64 * q;
      if (grank[q] == 0 || gcls[q] != c) continue;
      const double v = kind ? cm_mask_iou(irow[g], darea, garea[q]) : cm_box_iou(db, gbox[q]);
      if (v >= need && cm_replaces(grank[q], v, g, rank, iou, who)) { rank = grank[q]; iou = v; who = g; }
    }
    for (int off = 32; off > 0; off >>= 1) {      // butterfly: every lane ends with the winner
      const int r2 = __shfl_xor(rank, off), w2 = __shfl_xor(who, off);
      const double v2 = __shfl_xor(iou, off);
      if (r2 > 0 && cm_replaces(r2, v2, w2, rank, iou, who)) { rank = r2; iou = v2; who = w2; }
    }
    bool ig;
    if (rank > 0) {
      ig = rank == 1;
      if ((who & 63) == lane) grank[who >> 6] = 0;                   // matched: out of every later detection's walk
    } else {
      ig = cm_out_of_range(kind ? (double)darea : cm_box_area(db), a);
    }
    if (lane == 0) {
      if (rank > 0) s_m[pos >> 5] |= 1u << (pos & 31);
      if (ig) s_i[pos >> 5] |= 1u << (pos & 31);
    }
  }
  __syncthreads();
  const long long row = (((long long)t * CM_KINDS + kind) * CM_RANGES + a) * CM_THRS + ti;
  for (int w = lane; w < W; w += 64) {
    p.matched[row * W + w] = s_m[w];
    p.ignored[row * W + w] = s_i[w];
  }
}

// ---- the road cover vote (road_vote.h) ----

// One work item per cell (label g, class c) of tile blockIdx.y, neighbouring lanes on neighbouring labels: the walk over the tile's
// detection slots reads one row of `inter` per slot, coalesced, and the slot's class and score as one value for the wave.  No atomics:
// the cell has one owner and the slots come in ascending order.  The tables were zeroed by the launcher; a cell without a label, or
// of a label without area, stays as it is.
__global__ __launch_bounds__(256) void road_vote_kernel(const RoadVoteParams p) {
  const int t = blockIdx.y, cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= p.g_cap * p.K) return;
  const int c = cell / p.g_cap, g = cell - c * p.g_cap;
  if (g >= rv_tile_labels(p.tile_first, t, p.g_cap)) return;
  const int area = p.gt_area[(long long)t * p.g_cap + g];
  if (area <= 0) return;
  const int n = rv_tile_dets(p.det_count, t, p.D);
  const int* col = p.inter + (long long)t * p.D * p.g_cap + g;
  const int* cls = p.det_classes + (long long)t * p.D;
  const float* sc = p.det_scores + (long long)t * p.D;
  RvCell a;
  rv_clear(&a);
  for (int d = 0; d < n; ++d) rv_pair(&a, col[(long long)d * p.g_cap], area, cls[d], sc[d], c, p.threshold);
  const long long o = ((long long)t * p.g_cap + g) * p.K + c;
  p.wscore[o] = a.ws;
  p.wfrac[o] = a.wa;
  p.pairs[o] = a.pairs;
}

// The sweep (road_vote.h): road_vote_kernel's walk once per threshold.  blockIdx.z is the threshold's index, so thresholds[j] is read
// from the by-value parameters as one value for the whole workgroup and the compare of rv_pair is against a wave-uniform double; no
// array is indexed per lane, nothing lives in scratch.  The division of rv_frac is repeated per threshold: every slice walks the same
// slots with the same arithmetic as the single-threshold kernel, which is what makes slice j its tables bit for bit.
__global__ __launch_bounds__(256) void road_vote_sweep_kernel(const RoadVoteSweepParams p) {
  const int t = blockIdx.y, j = blockIdx.z, cell = blockIdx.x * 256 + threadIdx.x;
  if (j >= p.T || cell >= p.g_cap * p.K) return;
  const int c = cell / p.g_cap, g = cell - c * p.g_cap;
  if (g >= rv_tile_labels(p.tile_first, t, p.g_cap)) return;
  const int area = p.gt_area[(long long)t * p.g_cap + g];
  if (area <= 0) return;
  const double threshold = p.thresholds[j];
  const int n = rv_tile_dets(p.det_count, t, p.D);
  const int* col = p.inter + (long long)t * p.D * p.g_cap + g;
  const int* cls = p.det_classes + (long long)t * p.D;
  const float* sc = p.det_scores + (long long)t * p.D;
  RvCell a;
  rv_clear(&a);
  for (int d = 0; d < n; ++d) rv_pair(&a, col[(long long)d * p.g_cap], area, cls[d], sc[d], c, threshold);
  const long long o = (((long long)t * p.T + j) * p.g_cap + g) * p.K + c;
  p.wscore[o] = a.ws;
  p.wfrac[o] = a.wa;
  p.pairs[o] = a.pairs;
}

}  // namespace

int road_vote_check(const char* who, const RoadVoteParams& p) {
  RS_CHECK(p.det_scores && p.det_classes && p.det_count && p.tile_first && p.inter && p.gt_area && p.wscore && p.wfrac && p.pairs, RS_ERR_ARG,
           "%s: null table", who);
  RS_CHECK(p.n >= 1 && p.n <= 65535, RS_ERR_ARG, "%s: %d tiles (1..65535)", who, p.n);
  RS_CHECK(p.K >= 1 && p.K <= RV_MAX_CLASSES, RS_ERR_ARG, "%s: %d classes outside [1, %d]", who, p.K, RV_MAX_CLASSES);
  RS_CHECK(p.D >= 1 && p.g_cap >= 1, RS_ERR_ARG, "%s: %d slots, %d labels per tile", who, p.D, p.g_cap);
  RS_CHECK(p.threshold - p.threshold == 0.0, RS_ERR_ARG, "%s: the threshold is not finite", who);
  RS_CHECK(p.D <= RV_MAX_SLOTS, RS_ERR_UNSUPPORTED, "%s: %d slots per tile, the stage holds %d", who, p.D, RV_MAX_SLOTS);
  RS_CHECK(p.g_cap <= RV_MAX_GT, RS_ERR_UNSUPPORTED, "%s: gt_cap %d, the stage holds %d labels per tile", who, p.g_cap, RV_MAX_GT);
  return RS_OK;
}

int launch_road_votes(const RoadVoteParams& p, hipStream_t s) {
  { int rc = road_vote_check("road votes", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.g_cap * p.K;
  RS_HIP(hipMemsetAsync(p.wscore, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.wfrac, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.pairs, 0, cells * 4, s));
  hipLaunchKernelGGL(road_vote_kernel, dim3((unsigned)cdiv(p.g_cap * p.K, 256), (unsigned)p.n), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// The host restatement: the sequential loop over tiles, labels, classes and slots, on road_vote.h's per-pair rule.
int host_road_votes(const RoadVoteParams& p) {
  { int rc = road_vote_check("rs_host_road_votes", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.g_cap * p.K;
  memset(p.wscore, 0, cells * 8);
  memset(p.wfrac, 0, cells * 8);
  memset(p.pairs, 0, cells * 4);
  for (int t = 0; t < p.n; ++t) {
    const int G = rv_tile_labels(p.tile_first, t, p.g_cap), n = rv_tile_dets(p.det_count, t, p.D);
    for (int g = 0; g < G; ++g) {
      const int area = p.gt_area[(size_t)t * p.g_cap + g];
      if (area <= 0) continue;
      for (int c = 0; c < p.K; ++c) {
        RvCell a;
        rv_clear(&a);
        for (int d = 0; d < n; ++d)
          rv_pair(&a, p.inter[((size_t)t * p.D + d) * p.g_cap + g], area, p.det_classes[(size_t)t * p.D + d], p.det_scores[(size_t)t * p.D + d], c, p.threshold);
        const size_t o = ((size_t)t * p.g_cap + g) * p.K + c;
        p.wscore[o] = a.ws;
        p.wfrac[o] = a.wa;
        p.pairs[o] = a.pairs;
      }
    }
  }
  return RS_OK;
}

int road_vote_sweep_check(const char* who, const RoadVoteSweepParams& p) {
  RoadVoteParams q;
  memset(&q, 0, sizeof q);
  q.det_scores = p.det_scores; q.det_classes = p.det_classes; q.det_count = p.det_count; q.tile_first = p.tile_first; q.inter = p.inter;
  q.gt_area = p.gt_area; q.wscore = p.wscore; q.wfrac = p.wfrac; q.pairs = p.pairs; q.threshold = 0.0;
  q.n = p.n; q.K = p.K; q.D = p.D; q.g_cap = p.g_cap;
  { int rc = road_vote_check(who, q); if (rc) return rc; }
  RS_CHECK(p.T >= 1 && p.T <= RV_SWEEP_MAX, RS_ERR_ARG, "%s: %d thresholds outside [1, %d]", who, p.T, RV_SWEEP_MAX);
  for (int j = 0; j < p.T; ++j)
    RS_CHECK(p.thresholds[j] - p.thresholds[j] == 0.0, RS_ERR_ARG, "%s: threshold %d is not finite", who, j);
  return RS_OK;
}

int launch_road_votes_sweep(const RoadVoteSweepParams& p, hipStream_t s) {
  { int rc = road_vote_sweep_check("road vote sweep", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.T * p.g_cap * p.K;
  RS_HIP(hipMemsetAsync(p.wscore, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.wfrac, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.pairs, 0, cells * 4, s));
  hipLaunchKernelGGL(road_vote_sweep_kernel, dim3((unsigned)cdiv(p.g_cap * p.K, 256), (unsigned)p.n, (unsigned)p.T), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// The host restatement of the sweep: host_road_votes' loops once per threshold, slice by slice.
int host_road_votes_sweep(const RoadVoteSweepParams& p) {
  { int rc = road_vote_sweep_check("rs_host_road_votes_sweep", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.T * p.g_cap * p.K;
  memset(p.wscore, 0, cells * 8);
  memset(p.wfrac, 0, cells * 8);
  memset(p.pairs, 0, cells * 4);
  for (int t = 0; t < p.n; ++t) {
    const int G = rv_tile_labels(p.tile_first, t, p.g_cap), n = rv_tile_dets(p.det_count, t, p.D);
    for (int j = 0; j < p.T; ++j) {
      const double threshold = p.thresholds[j];
      for (int g = 0; g < G; ++g) {
        const int area = p.gt_area[(size_t)t * p.g_cap + g];
        if (area <= 0) continue;
        for (int c = 0; c < p.K; ++c) {
          RvCell a;
          rv_clear(&a);
          for (int d = 0; d < n; ++d)
            rv_pair(&a, p.inter[((size_t)t * p.D + d) * p.g_cap + g], area, p.det_classes[(size_t)t * p.D + d], p.det_scores[(size_t)t * p.D + d], c, threshold);
          const size_t o = (((size_t)t * p.T + j) * p.g_cap + g) * p.K + c;
          p.wscore[o] = a.ws;
          p.wfrac[o] = a.wa;
          p.pairs[o] = a.pairs;
        }
      }
    }
  }
  return RS_OK;
}

int coco_match_check(const char* who, const CocoMatchParams& p) {
  RS_CHECK(p.det_boxes && p.det_scores && p.det_classes && p.det_count && p.gt_boxes && p.gt_classes && p.tile_first && p.inter && p.det_area && p.gt_area && p.order &&
           p.class_first && p.gt_per_class && p.matched && p.ignored && p.npig, RS_ERR_ARG, "%s: null table", who);
  RS_CHECK(p.n >= 1 && p.n <= 65535, RS_ERR_ARG, "%s: %d tiles (1..65535)", who, p.n);
  RS_CHECK(p.K >= 1 && p.K <= CM_MAX_CLASSES, RS_ERR_ARG, "%s: %d classes outside [1, %d]", who, p.K, CM_MAX_CLASSES);
  RS_CHECK(p.D >= 1 && p.g_cap >= 1, RS_ERR_ARG, "%s: %d slots, %d ground truths per tile", who, p.D, p.g_cap);
  RS_CHECK(p.D <= CM_MAX_SLOTS, RS_ERR_UNSUPPORTED, "%s: %d slots per tile, the kernels hold %d", who, p.D, CM_MAX_SLOTS);
  RS_CHECK(p.g_cap <= CM_MAX_GT, RS_ERR_UNSUPPORTED, "%s: gt_cap %d, the kernels hold %d ground truths per tile", who, p.g_cap, CM_MAX_GT);
  return RS_OK;
}

int launch_coco_match(const CocoMatchParams& p, hipStream_t s) {
  { int rc = coco_match_check("coco match", p); if (rc) return rc; }
  hipLaunchKernelGGL(coco_order_kernel, dim3((unsigned)p.n), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  hipLaunchKernelGGL(coco_match_kernel, dim3(CM_KINDS * CM_RANGES * CM_THRS, (unsigned)p.n), dim3(64), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// The host restatement: coco_eval.match_images / _evaluate_img as plain loops over coco_match.h's per-element rules.  The order is
// built by the kernel's counting rule; the greedy walk is Python's own (kept ground truths, then ignored ones, `best` carried along,
// the early stop), not the kernel's reduction.
int host_coco_match(const CocoMatchParams& p) {
  { int rc = coco_match_check("rs_host_coco_match", p); if (rc) return rc; }
  const int K = p.K, D = p.D, W = (D + 31) >> 5, cap = p.g_cap;
  for (int t = 0; t < p.n; ++t) {
    const int n = p.det_count[t] > D ? D : (p.det_count[t] < 0 ? 0 : p.det_count[t]);
    const int g0 = p.tile_first[t];
    int G = p.tile_first[t + 1] - g0;
    G = G > cap ? cap : (G < 0 ? 0 : G);
    const int* cls = p.det_classes + (size_t)t * D;
    const float* sc = p.det_scores + (size_t)t * D;
    int* order = p.order + (size_t)t * D;
    int* first = p.class_first + (size_t)t * (K + 1);
    for (int i = 0; i < D; ++i) order[i] = -1;
    for (int i = 0; i < n; ++i) {
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += cm_before(cm_class(cls[j], K), sc[j], j, cm_class(cls[i], K), sc[i], i);
      order[rank] = i;
    }
    for (int c = 0; c <= K; ++c) {
      first[c] = 0;
      for (int j = 0; j < n; ++j) first[c] += cm_class(cls[j], K) < c;
    }
    for (int c = 0; c < K; ++c) {
      int k = 0;
      for (int g = 0; g < G; ++g) k += p.gt_classes[g0 + g] == c;
      p.gt_per_class[(size_t)t * K + c] = k;
    }
    for (int kind = 0; kind < CM_KINDS; ++kind)
      for (int a = 0; a < CM_RANGES; ++a) {
        bool ign[CM_MAX_GT];
        int walk[CM_MAX_GT];                      // np.argsort(g_ignore, kind="mergesort"): kept ones first, each group in order
        int nw = 0;
        for (int g = 0; g < G; ++g)
          ign[g] = cm_out_of_range(kind ? (double)p.gt_area[(size_t)t * cap + g] : cm_box_area(p.gt_boxes + 4 * (size_t)(g0 + g)), a);
        for (int pass = 0; pass < 2; ++pass)
          for (int g = 0; g < G; ++g)
            if (ign[g] == (pass == 1)) walk[nw++] = g;
        int* npig = p.npig + (((size_t)t * CM_KINDS + kind) * CM_RANGES + a) * K;
        for (int c = 0; c < K; ++c) {
          npig[c] = 0;
          for (int g = 0; g < G; ++g) npig[c] += p.gt_classes[g0 + g] == c && !ign[g];
        }
        for (int ti = 0; ti < CM_THRS; ++ti) {
          const size_t row = ((((size_t)t * CM_KINDS + kind) * CM_RANGES + a) * CM_THRS + ti) * W;
          for (int w = 0; w < W; ++w) p.matched[row + w] = p.ignored[row + w] = 0;
          bool gtm[CM_MAX_GT] = {false};
          for (int pos = 0; pos < n; ++pos) {
            const int slot = order[pos];
            if (slot < 0) continue;
            const int c = cls[slot];
            if (c < 0 || c >= K) continue;
            double db[4];
            for (int k = 0; k < 4; ++k) db[k] = (double)p.det_boxes[((size_t)t * D + slot) * 4 + k];
            const int darea = p.det_area[(size_t)t * D + slot];
            double best = cm_floor(p.thrs[ti]);
            int m = -1;
            for (int wi = 0; wi < nw; ++wi) {
              const int g = walk[wi];
              if (p.gt_classes[g0 + g] != c || gtm[g]) continue;
              if (m > -1 && !ign[m] && ign[g]) break;
              const double v = kind ? cm_mask_iou(p.inter[((size_t)t * D + slot) * cap + g], darea, p.gt_area[(size_t)t * cap + g])
                                    : cm_box_iou(db, p.gt_boxes + 4 * (size_t)(g0 + g));
              if (v < best) continue;
              best = v; m = g;
            }
            bool ig;
            if (m > -1) {
              gtm[m] = true;
              ig = ign[m];
              p.matched[row + (pos >> 5)] |= 1u << (pos & 31);
            } else {
              ig = cm_out_of_range(kind ? (double)darea : cm_box_area(db), a);
            }
            if (ig) p.ignored[row + (pos >> 5)] |= 1u << (pos & 31);
          }
        }
      }
  }
  return RS_OK;
}

int launch_canvas_raster(const CanvasRasterParams& p, hipStream_t s) {
  RS_CHECK(p.inst_first && p.out && p.n_inst >= 0, RS_ERR_ARG, "canvas raster: null table");
  RS_CHECK(p.side >= 1 && p.side <= CR_MAX_SIDE, RS_ERR_ARG, "canvas raster: side %d outside [1, %d]", p.side, CR_MAX_SIDE);
  RS_CHECK(p.n_inst <= 65535, RS_ERR_ARG, "canvas raster: %d instances in one launch (at most 65535)", p.n_inst);
  if (p.n_inst == 0) return RS_OK;
  hipLaunchKernelGGL(canvas_raster_kernel, dim3((unsigned)cdiv(p.side, CR_STRIP), (unsigned)p.n_inst), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_mask_pair_counts(const PairCountParams& p, hipStream_t s) {
  RS_CHECK(p.det_masks && p.det_count && p.tile_first && p.inter && p.det_area && p.gt_area, RS_ERR_ARG, "mask pair counts: null buffer");
  RS_CHECK(p.n >= 1 && p.n <= 65535 && p.D >= 1 && p.g_cap >= 1 && p.bytes > 0, RS_ERR_ARG, "mask pair counts: bad argument");
  RS_CHECK(p.bytes % 4 == 0 && p.bytes / 4 <= 0x7fffffffll, RS_ERR_UNSUPPORTED, "mask pair counts: %lld bytes per mask must be a multiple of 4", p.bytes);
  RS_HIP(hipMemsetAsync(p.inter, 0, (size_t)p.n * p.D * p.g_cap * 4, s));
  RS_HIP(hipMemsetAsync(p.det_area, 0, (size_t)p.n * p.D * 4, s));
  RS_HIP(hipMemsetAsync(p.gt_area, 0, (size_t)p.n * p.g_cap * 4, s));
  hipLaunchKernelGGL(mask_pair_counts_kernel, dim3((unsigned)p.D + 1, (unsigned)p.n), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}
