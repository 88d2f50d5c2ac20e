// The road cover vote on polygon areas ("polygon geometry").
//   poly_overlap_kernel          area(label ∩ detection) / area(label), rounded to two decimals, for every pair of every tile of a
//                                batch: the closed-form edge-pair sum of poly_overlap.h on the polygoniser's int16 vertex tables and
//                                the labels' float64 rings.  One workgroup per (tile, label); float64, no atomics on floats.
//   road_vote_area_sweep_kernel  road_vote_sweep_kernel's walk (val_ap.hip) reading those weights: rv_pair_area of road_vote.h.
// host_poly_overlaps and host_road_votes_area_sweep are the same rules as plain host loops in the kernels' summation order
// (rs_host_polygon_overlaps, rs_host_road_votes_area_sweep); they live here for the compile flags (no mul+add contraction).
#include <string.h>

#include "poly_vote.h"

namespace {

constexpr int PV_THREADS = 256;
constexpr int PV_WAVES = PV_THREADS / PO_LANES;

// One workgroup per (label g = blockIdx.x, tile t = blockIdx.y).  Thread 0 scans the label (box, origin, area: sequential, as the host);
// the label's edge slots are staged in LDS a chunk of PO_STAGE at a time, one thread per ring; the four waves take the tile's
// detections d = wave, wave + 4, ...: a wave leaves a detection on the flag, the empty instance and the box test, otherwise walks its
// rings with the edges strided over the lanes, every lane running over the staged label edges (all lanes read the same LDS address: a
// broadcast), and sums the lanes with the butterfly of poly_overlap.h.  Lane 0 owns the pair's cell of `frac`: it holds the area until
// the last chunk is in, then the rounded weight.  Every loop bound is read before its loop starts.
__global__ __launch_bounds__(PV_THREADS) void poly_overlap_kernel(const PolyOverlapParams p) {
  __shared__ double s_edge[PO_STAGE][5];
  __shared__ PoLabel s_lab;
  __shared__ int s_flagged;
  const int t = blockIdx.y, g = blockIdx.x, tid = threadIdx.x, lane = tid & (PO_LANES - 1), wave = tid / PO_LANES;
  const int nd = rv_tile_dets(p.det_count, t, p.D);
  const int* hdr = p.header + (long long)t * p.D * PO_HDR;
  if (g == 0) {      // the tile's flagged instances: integers, any order
    if (tid == 0) s_flagged = 0;
    __syncthreads();
    int mine = 0;
    for (int d = tid; d < nd; d += PV_THREADS) mine += hdr[d * PO_HDR] != 0;
    if (mine) atomicAdd(&s_flagged, mine);
    __syncthreads();
    if (tid == 0) p.flagged[t] = s_flagged;
  }
  if (g >= rv_tile_labels(p.tile_first, t, p.g_cap)) return;
  const int inst = p.tile_first[t] + g;
  const int r0 = p.inst_first[inst], r1 = p.inst_first[inst + 1];
  if (tid == 0) {
    PoLabel L;
    po_label_scan(&L, p.polys, p.poly_off, p.poly_len, r0, r1);
    s_lab = L;
    p.label_area[(long long)t * p.g_cap + g] = L.area;
  }
  __syncthreads();
  const PoLabel L = s_lab;
  if (!(L.area > 0.0) || L.slots <= 0) return;
  double* cell = p.frac + (long long)t * p.D * p.g_cap + g;      // cell[d * g_cap]
  const int chunks = (L.slots + PO_STAGE - 1) / PO_STAGE;
  for (int c = 0; c < chunks; ++c) {
    const int lo = c * PO_STAGE, cnt = L.slots - lo < PO_STAGE ? L.slots - lo : PO_STAGE;
    if (c) __syncthreads();                                       // the readers of the chunk before are done
    for (int r = r0 + tid; r < r1; r += PV_THREADS) {             // one thread per ring: its slots that fall into [lo, lo + cnt)
      int first = 0;
      for (int q = r0; q < r; ++q) first += p.poly_len[q] / 2 > 0 ? p.poly_len[q] / 2 : 0;
      const int n = p.poly_len[r] / 2;
      const int i0 = lo - first > 0 ? lo - first : 0, i1 = lo + cnt - first < n ? lo + cnt - first : n;
      if (i0 >= i1) continue;
      const double* ring = p.polys + p.poly_off[r];
      const double sh = po_ring_shoelace(ring, n, L.ox, L.oy);
      for (int i = i0; i < i1; ++i) {
        PoEdge e;
        po_label_edge(&e, ring, n, i, sh, L.ox, L.oy);
        double* o = s_edge[first + i - lo];
        o[0] = e.xl; o[1] = e.xr; o[2] = e.yl; o[3] = e.m; o[4] = e.s;
      }
    }
    __syncthreads();
    for (int d = wave; d < nd; d += PV_WAVES) {
      const int* h = hdr + d * PO_HDR;
      const int flagged = h[0], np = h[1], nv = h[3], p0 = h[4], q0 = h[5], v0 = h[6];
      if (flagged || np <= 0 || nv <= 0) continue;
      int xmin = 32767, xmax = -32768, ymin = 32767, ymax = -32768;
      for (int v = lane; v < nv; v += PO_LANES) {
        const int x = p.xy[2 * (v0 + v)], y = p.xy[2 * (v0 + v) + 1];
        xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax; ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
      }
      for (int off = 32; off >= 1; off >>= 1) {
        const int a = __shfl_xor(xmin, off), b = __shfl_xor(xmax, off), cc = __shfl_xor(ymin, off), dd = __shfl_xor(ymax, off);
        xmin = a < xmin ? a : xmin; xmax = b > xmax ? b : xmax; ymin = cc < ymin ? cc : ymin; ymax = dd > ymax ? dd : ymax;
      }
      if (!po_boxes_meet(L, xmin, xmax, ymin, ymax)) continue;
      double acc = 0.0;
      int ring = q0, vert = v0;
      for (int pi = 0; pi < np; ++pi) {
        const int nr = p.poly_ring_count[p0 + pi];
        for (int ri = 0; ri < nr; ++ri, ++ring) {
          const int len = p.ring_len[ring], ne = len - 1;
          long long sh = 0;
          for (int k = lane; k < ne; k += PO_LANES) sh += po_det_cross(p.xy, vert + k);
          for (int off = 32; off >= 1; off >>= 1) sh += __shfl_xor(sh, off);
          for (int k = lane; k < ne; k += PO_LANES) {
            PoEdge f;
            po_det_edge(&f, p.xy, vert, k, ri == 0 ? 1 : -1, sh, L.ox, L.oy);
            double row = 0.0;
            for (int j = 0; j < cnt; ++j) {
              PoEdge e;
              e.xl = s_edge[j][0]; e.xr = s_edge[j][1]; e.yl = s_edge[j][2]; e.m = s_edge[j][3]; e.s = s_edge[j][4];
              row += po_pair(e, f);
            }
            acc += row;
          }
          vert += len > 0 ? len : 0;
        }
      }
      for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
      if (lane == 0) {
        double* o = cell + (long long)d * p.g_cap;
        *o = c ? *o + acc : acc;
      }
    }
  }
  if (p.raw_areas) return;
  for (int d = wave; d < nd; d += PV_WAVES)          // the same lane that wrote the areas turns them into weights
    if (lane == 0) {
      double* o = cell + (long long)d * p.g_cap;
      *o = po_frac(*o, L.area);
    }
}

// road_vote_sweep_kernel's shape: one work item per cell (label g, class c) of tile blockIdx.y and threshold blockIdx.z, neighbouring
// lanes on neighbouring labels, one coalesced row of `frac` per slot.  A cell without a label stays zero (the launcher cleared it).
__global__ __launch_bounds__(256) void road_vote_area_sweep_kernel(const RoadVoteAreaSweepParams p) {
  const int t = blockIdx.y, j = blockIdx.z, cellx = blockIdx.x * 256 + threadIdx.x;
  if (j >= p.T || cellx >= p.g_cap * p.K) return;
  const int c = cellx / p.g_cap, g = cellx - c * p.g_cap;
  if (g >= rv_tile_labels(p.tile_first, t, p.g_cap)) return;
  const double threshold = p.thresholds[j];
  const int n = rv_tile_dets(p.det_count, t, p.D);
  const double* col = p.frac + (long long)t * p.D * p.g_cap + g;
  const int* cls = p.det_classes + (long long)t * p.D;
  const float* sc = p.det_scores + (long long)t * p.D;
  RvCell a;
  rv_clear(&a);
  for (int d = 0; d < n; ++d) rv_pair_area(&a, col[(long long)d * p.g_cap], cls[d], sc[d], c, threshold);
  const long long o = (((long long)t * p.T + j) * p.g_cap + g) * p.K + c;
  p.wscore[o] = a.ws;
  p.wfrac[o] = a.wa;
  p.pairs[o] = a.pairs;
}

}  // namespace

int poly_overlap_check(const char* who, const PolyOverlapParams& p) {
  RS_CHECK(p.header && p.poly_ring_count && p.ring_len && p.xy && p.det_count && p.tile_first && p.inst_first && p.poly_off && p.poly_len && p.polys &&
           p.frac && p.label_area && p.flagged, RS_ERR_ARG, "%s: null table", who);
  RS_CHECK(p.n >= 1 && p.n <= 65535, RS_ERR_ARG, "%s: %d tiles (1..65535)", who, p.n);
  RS_CHECK(p.D >= 1 && p.g_cap >= 1, RS_ERR_ARG, "%s: %d slots, %d labels per tile", who, p.D, p.g_cap);
  RS_CHECK(p.D <= RV_MAX_SLOTS, RS_ERR_UNSUPPORTED, "%s: %d slots per tile, the stage holds %d", who, p.D, RV_MAX_SLOTS);
  RS_CHECK(p.g_cap <= RV_MAX_GT, RS_ERR_UNSUPPORTED, "%s: gt_cap %d, the stage holds %d labels per tile", who, p.g_cap, RV_MAX_GT);
  return RS_OK;
}

int launch_poly_overlaps(const PolyOverlapParams& p, hipStream_t s) {
  { int rc = poly_overlap_check("polygon overlaps", p); if (rc) return rc; }
  RS_HIP(hipMemsetAsync(p.frac, 0, (size_t)p.n * p.D * p.g_cap * 8, s));
  RS_HIP(hipMemsetAsync(p.label_area, 0, (size_t)p.n * p.g_cap * 8, s));
  RS_HIP(hipMemsetAsync(p.flagged, 0, (size_t)p.n * 4, s));
  hipLaunchKernelGGL(poly_overlap_kernel, dim3((unsigned)p.g_cap, (unsigned)p.n), dim3(PV_THREADS), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// The host restatement: the kernel's loops with the 64 lane accumulators as an array (poly_overlap.h, SUMMATION ORDER).
int host_poly_overlaps(const PolyOverlapParams& p) {
  { int rc = poly_overlap_check("rs_host_polygon_overlaps", p); if (rc) return rc; }
  memset(p.frac, 0, (size_t)p.n * p.D * p.g_cap * 8);
  memset(p.label_area, 0, (size_t)p.n * p.g_cap * 8);
  memset(p.flagged, 0, (size_t)p.n * 4);
  static thread_local PoEdge stage[PO_STAGE];
  for (int t = 0; t < p.n; ++t) {
    const int G = rv_tile_labels(p.tile_first, t, p.g_cap), nd = rv_tile_dets(p.det_count, t, p.D);
    const int* hdr = p.header + (size_t)t * p.D * PO_HDR;
    for (int d = 0; d < nd; ++d) p.flagged[t] += hdr[d * PO_HDR] != 0;
    for (int g = 0; g < G; ++g) {
      const int inst = p.tile_first[t] + g;
      const int r0 = p.inst_first[inst], r1 = p.inst_first[inst + 1];
      PoLabel L;
      po_label_scan(&L, p.polys, p.poly_off, p.poly_len, r0, r1);
      p.label_area[(size_t)t * p.g_cap + g] = L.area;
      if (!(L.area > 0.0) || L.slots <= 0) continue;
      double* cell = p.frac + (size_t)t * p.D * p.g_cap + g;
      const int chunks = (L.slots + PO_STAGE - 1) / PO_STAGE;
      for (int c = 0; c < chunks; ++c) {
        const int lo = c * PO_STAGE, cnt = L.slots - lo < PO_STAGE ? L.slots - lo : PO_STAGE;
        int first = 0;
        for (int r = r0; r < r1; ++r) {
          const int n = p.poly_len[r] / 2;
          const int i0 = lo - first > 0 ? lo - first : 0, i1 = lo + cnt - first < n ? lo + cnt - first : n;
          if (i0 < i1) {
            const double* ring = p.polys + p.poly_off[r];
            const double sh = po_ring_shoelace(ring, n, L.ox, L.oy);
            for (int i = i0; i < i1; ++i) po_label_edge(&stage[first + i - lo], ring, n, i, sh, L.ox, L.oy);
          }
          first += n > 0 ? n : 0;
        }
        for (int d = 0; d < nd; ++d) {
          const int* h = hdr + d * PO_HDR;
          const int flagged = h[0], np = h[1], nv = h[3], p0 = h[4], q0 = h[5], v0 = h[6];
          if (flagged || np <= 0 || nv <= 0) continue;
          int xmin = 32767, xmax = -32768, ymin = 32767, ymax = -32768;
          for (int v = 0; v < nv; ++v) {
            const int x = p.xy[2 * (v0 + v)], y = p.xy[2 * (v0 + v) + 1];
            xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax; ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
          }
          if (!po_boxes_meet(L, xmin, xmax, ymin, ymax)) continue;
          double acc[PO_LANES];
          for (int l = 0; l < PO_LANES; ++l) acc[l] = 0.0;
          int ring = q0, vert = v0;
          for (int pi = 0; pi < np; ++pi) {
            const int nr = p.poly_ring_count[p0 + pi];
            for (int ri = 0; ri < nr; ++ri, ++ring) {
              const int len = p.ring_len[ring], ne = len - 1;
              long long sh = 0;
              for (int k = 0; k < ne; ++k) sh += po_det_cross(p.xy, vert + k);
              for (int k = 0; k < ne; ++k) {
                PoEdge f;
                po_det_edge(&f, p.xy, vert, k, ri == 0 ? 1 : -1, sh, L.ox, L.oy);
                double row = 0.0;
                for (int j = 0; j < cnt; ++j) row += po_pair(stage[j], f);
                acc[k & (PO_LANES - 1)] += row;
              }
              vert += len > 0 ? len : 0;
            }
          }
          for (int off = 32; off >= 1; off >>= 1)
            for (int l = 0; l < off; ++l) acc[l] = acc[l] + acc[l + off];
          double* o = cell + (size_t)d * p.g_cap;
          *o = c ? *o + acc[0] : acc[0];
        }
      }
      for (int d = 0; d < nd && !p.raw_areas; ++d) {
        double* o = cell + (size_t)d * p.g_cap;
        *o = po_frac(*o, L.area);
      }
    }
  }
  return RS_OK;
}

int road_vote_area_sweep_check(const char* who, const RoadVoteAreaSweepParams& p) {
  RS_CHECK(p.det_scores && p.det_classes && p.det_count && p.tile_first && p.frac && p.wscore && p.wfrac && p.pairs, RS_ERR_ARG, "%s: null table", who);
  RS_CHECK(p.n >= 1 && p.n <= 65535, RS_ERR_ARG, "%s: %d tiles (1..65535)", who, p.n);
  RS_CHECK(p.K >= 1 && p.K <= RV_MAX_CLASSES, RS_ERR_ARG, "%s: %d classes outside [1, %d]", who, p.K, RV_MAX_CLASSES);
  RS_CHECK(p.D >= 1 && p.g_cap >= 1, RS_ERR_ARG, "%s: %d slots, %d labels per tile", who, p.D, p.g_cap);
  RS_CHECK(p.D <= RV_MAX_SLOTS, RS_ERR_UNSUPPORTED, "%s: %d slots per tile, the stage holds %d", who, p.D, RV_MAX_SLOTS);
  RS_CHECK(p.g_cap <= RV_MAX_GT, RS_ERR_UNSUPPORTED, "%s: gt_cap %d, the stage holds %d labels per tile", who, p.g_cap, RV_MAX_GT);
  RS_CHECK(p.T >= 1 && p.T <= RV_SWEEP_MAX, RS_ERR_ARG, "%s: %d thresholds outside [1, %d]", who, p.T, RV_SWEEP_MAX);
  for (int j = 0; j < p.T; ++j)
    RS_CHECK(p.thresholds[j] - p.thresholds[j] == 0.0, RS_ERR_ARG, "%s: threshold %d is not finite", who, j);
  return RS_OK;
}

int launch_road_votes_area_sweep(const RoadVoteAreaSweepParams& p, hipStream_t s) {
  { int rc = road_vote_area_sweep_check("road vote area sweep", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.T * p.g_cap * p.K;
  RS_HIP(hipMemsetAsync(p.wscore, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.wfrac, 0, cells * 8, s));
  RS_HIP(hipMemsetAsync(p.pairs, 0, cells * 4, s));
  hipLaunchKernelGGL(road_vote_area_sweep_kernel, dim3((unsigned)cdiv(p.g_cap * p.K, 256), (unsigned)p.n, (unsigned)p.T), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int host_road_votes_area_sweep(const RoadVoteAreaSweepParams& p) {
  { int rc = road_vote_area_sweep_check("rs_host_road_votes_area_sweep", p); if (rc) return rc; }
  const size_t cells = (size_t)p.n * p.T * p.g_cap * p.K;
  memset(p.wscore, 0, cells * 8);
  memset(p.wfrac, 0, cells * 8);
  memset(p.pairs, 0, cells * 4);
  for (int t = 0; t < p.n; ++t) {
    const int G = rv_tile_labels(p.tile_first, t, p.g_cap), n = rv_tile_dets(p.det_count, t, p.D);
    for (int j = 0; j < p.T; ++j) {
      const double threshold = p.thresholds[j];
      for (int g = 0; g < G; ++g)
        for (int c = 0; c < p.K; ++c) {
          RvCell a;
          rv_clear(&a);
          for (int d = 0; d < n; ++d)
            rv_pair_area(&a, p.frac[((size_t)t * p.D + d) * p.g_cap + g], p.det_classes[(size_t)t * p.D + d], p.det_scores[(size_t)t * p.D + d], c, threshold);
          const size_t o = (((size_t)t * p.T + j) * p.g_cap + g) * p.K + c;
          p.wscore[o] = a.ws;
          p.wfrac[o] = a.wa;
          p.pairs[o] = a.pairs;
        }
    }
  }
  return RS_OK;
}
