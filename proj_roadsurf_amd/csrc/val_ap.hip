// Validation AP on the device: the two kernels between the engine's bit-packed detection masks and the integer
// tables coco_eval.match_images takes for `segm`.
//   canvas_raster_kernel      ground-truth polygons -> bit-packed canvases, bit for bit the host's rs_rasterize_polygons_within_box at
//                             box (0, 0, side, side): the per-column closed form of canvas_raster.h, fp64 in the host's operand order
//                             (compiled without mul+add contraction), integer LDS atomics only.
//   mask_pair_counts_kernel   popcounts of detection AND ground truth for every pair of every tile of a batch, with both sides' own
//                             areas.  Integers only.
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

}  // namespace

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
