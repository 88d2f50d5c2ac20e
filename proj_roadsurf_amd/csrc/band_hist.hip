// Band histograms under road labels (band_hist.h): what the reference's statistical route collects per road
// with rasterio.mask and a pandas frame of one row per pixel, counted behind the forward from the uint8 tiles and the label canvases
// that are on the device already.
//   band_hist_kernel          one workgroup per (label instance, chunk of 2048 canvas words).  The canvas is read as 32-bit words, a
//                             workgroup whose words are all zero leaves at once, a set bit reads its pixel's C bytes from the interleaved
//                             tile.  Counts go to LDS histograms private to each of the four waves (integer LDS atomics), so that
//                             a uniform tile under a full label serialises within a wave only; the copies are summed and published
//                             with plain stores where the workgroup owns the instance's rows (one chunk) and with integer global adds
//                             of the non-zero bins where the label is split over several workgroups.  Integer sums do not depend on
//                             the order of arrival: the bits are the same either way.  No float, no division.
// host_band_hist is the same rule as plain host loops (rs_host_band_hist).
#include <string.h>

#include "val_ap.h"

namespace {

constexpr int BH_THREADS = 256;
constexpr int BH_WAVES = BH_THREADS / 64;
constexpr int BH_WORDS = 8;                              // canvas words per work item
constexpr int BH_CHUNK = BH_THREADS * BH_WORDS;          // canvas words per workgroup: a side of 512 is 4 chunks, of 1024 16

// words: 32-bit words per canvas; chunks: workgroups per instance; steps: iterations that bisect n + 1 table entries down to one tile.
template <int C>
__global__ __launch_bounds__(BH_THREADS) void band_hist_kernel(const BandHistParams p, const int words, const int chunks, const int steps,
                                                               const unsigned long long magic) {
  __shared__ unsigned h[BH_WAVES * C * BH_BINS];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int first = blockIdx.y * BH_CHUNK + tid;          // this work item's words: first + i * BH_THREADS, coalesced
  const uint32_t* canvas = (const uint32_t*)p.label_masks + (size_t)g * words;
  uint32_t w[BH_WORDS];
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < BH_WORDS; ++i) {
    const int idx = first + i * BH_THREADS;
    w[i] = idx < words ? canvas[idx] : 0u;
    any |= w[i];
  }
  // nothing of the label in this chunk (most chunks of a road-shaped label): the launcher cleared the rows, in both ways of publishing
  if (!__syncthreads_or(any != 0)) return;

  // the tile that owns instance g: the last t with tile_first[t] <= g (tiles without labels repeat an entry and are stepped over)
  int lo = 0, hi = p.n;
  for (int i = 0; i < steps; ++i) {
    const int mid = (lo + hi) >> 1;
    if (mid > lo) {
      if (p.tile_first[mid] <= g) lo = mid; else hi = mid;
    }
  }
  const uint8_t* tile = p.tiles + (size_t)lo * p.side * p.side * C;

  for (int i = tid; i < BH_WAVES * C * BH_BINS; i += BH_THREADS) h[i] = 0u;
  __syncthreads();

  unsigned* mine = h + (tid >> 6) * (C * BH_BINS);
  const unsigned row_bytes = (unsigned)bh_row_bytes(p.side), side = (unsigned)p.side;
#pragma unroll
  for (int i = 0; i < BH_WORDS; ++i) {
    uint32_t word = w[i];
    const unsigned byte0 = (unsigned)(first + i * BH_THREADS) * 4u;
    const int bits = __popc(word);
    for (int k = 0; k < bits; ++k) {
      const unsigned bit = (unsigned)__ffs((int)word) - 1u;
      word &= word - 1u;
      const unsigned b = byte0 + (bit >> 3);            // little endian: bits 8j .. 8j + 7 of the word are byte j
      const unsigned y = bh_row_of(b, magic);           // < side: b < side * row_bytes
      const unsigned x = ((b - y * row_bytes) << 3) + (bit & 7u);
      if (x >= side) continue;                          // a padding bit of the row's last byte
      const uint8_t* px = tile + (size_t)(y * side + x) * C;
      unsigned v[C];
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = px[c];
      unsigned data = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) data |= v[c];
      if (!data) continue;                              // bh_has_data: every band 0 is nodata
#pragma unroll
      for (int c = 0; c < C; ++c) atomicAdd(&mine[c * BH_BINS + v[c]], 1u);
    }
  }
  __syncthreads();

  uint32_t* out = p.hist + (size_t)g * (C * BH_BINS);
  for (int i = tid; i < C * BH_BINS; i += BH_THREADS) {
    unsigned s = 0;
#pragma unroll
    for (int wv = 0; wv < BH_WAVES; ++wv) s += h[wv * (C * BH_BINS) + i];
    if (chunks == 1) out[i] = s;
    else if (s) atomicAdd(&out[i], s);
  }
}

}  // namespace

int band_hist_check(const char* who, const BandHistParams& p) {
  RS_CHECK(p.n_inst >= 0, RS_ERR_ARG, "%s: n_inst %d is negative", who, p.n_inst);
  RS_CHECK(p.tiles && p.tile_first && (p.n_inst == 0 || (p.label_masks && p.hist)), RS_ERR_ARG, "%s: null table", who);
  RS_CHECK(p.n >= 1, RS_ERR_ARG, "%s: n_tiles %d (at least 1)", who, p.n);
  RS_CHECK(p.side >= 1 && p.side <= BH_MAX_SIDE, RS_ERR_ARG, "%s: side %d outside [1, %d]", who, p.side, BH_MAX_SIDE);
  RS_CHECK(p.C >= 1 && p.C <= BH_MAX_CHANNELS, RS_ERR_ARG, "%s: channels %d outside [1, %d]", who, p.C, BH_MAX_CHANNELS);
  RS_CHECK(bh_canvas_bytes(p.side) % 4 == 0, RS_ERR_UNSUPPORTED, "%s: side %d gives canvases of %lld bytes, they must be a multiple of 4", who, p.side,
           bh_canvas_bytes(p.side));
  return RS_OK;
}

int launch_band_hist(const BandHistParams& p, hipStream_t s) {
  { int rc = band_hist_check("band histograms", p); if (rc) return rc; }
  if (p.n_inst == 0) return RS_OK;
  RS_CHECK(((uintptr_t)p.label_masks & 3) == 0, RS_ERR_ARG, "band histograms: the canvases are read as 32-bit words and must be 4-byte aligned");
  RS_HIP(hipMemsetAsync(p.hist, 0, (size_t)p.n_inst * p.C * BH_BINS * 4, s));
  const int words = (int)(bh_canvas_bytes(p.side) / 4), chunks = cdiv(words, BH_CHUNK);
  int steps = 1;
  while ((1ll << steps) < (long long)p.n + 1) ++steps;
  const unsigned long long magic = bh_row_magic(bh_row_bytes(p.side));
  const dim3 grid((unsigned)p.n_inst, (unsigned)chunks), block(BH_THREADS);
  switch (p.C) {
    case 1: hipLaunchKernelGGL(band_hist_kernel<1>, grid, block, 0, s, p, words, chunks, steps, magic); break;
    case 2: hipLaunchKernelGGL(band_hist_kernel<2>, grid, block, 0, s, p, words, chunks, steps, magic); break;
    case 3: hipLaunchKernelGGL(band_hist_kernel<3>, grid, block, 0, s, p, words, chunks, steps, magic); break;
    default: hipLaunchKernelGGL(band_hist_kernel<4>, grid, block, 0, s, p, words, chunks, steps, magic); break;
  }
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// The host restatement: the sequential loop over tiles, their labels, rows and pixels, on band_hist.h's rule.
int host_band_hist(const BandHistParams& p) {
  { int rc = band_hist_check("rs_host_band_hist", p); if (rc) return rc; }
  if (p.n_inst == 0) return RS_OK;
  memset(p.hist, 0, (size_t)p.n_inst * p.C * BH_BINS * 4);
  const int row_bytes = bh_row_bytes(p.side);
  const size_t canvas_bytes = (size_t)bh_canvas_bytes(p.side);
  for (int t = 0; t < p.n; ++t) {
    const uint8_t* tile = p.tiles + (size_t)t * p.side * p.side * p.C;
    const int g0 = p.tile_first[t] < 0 ? 0 : p.tile_first[t], g1 = p.tile_first[t + 1] > p.n_inst ? p.n_inst : p.tile_first[t + 1];
    for (int g = g0; g < g1; ++g) {
      const uint8_t* canvas = p.label_masks + (size_t)g * canvas_bytes;
      uint32_t* out = p.hist + (size_t)g * p.C * BH_BINS;
      for (int y = 0; y < p.side; ++y)
        for (int x = 0; x < p.side; ++x) {
          if (!((canvas[(size_t)y * row_bytes + (x >> 3)] >> (x & 7)) & 1)) continue;
          const uint8_t* px = tile + ((size_t)y * p.side + x) * p.C;
          if (!bh_has_data(px, p.C)) continue;
          for (int c = 0; c < p.C; ++c) out[c * BH_BINS + px[c]] += 1u;
        }
    }
  }
  return RS_OK;
}
