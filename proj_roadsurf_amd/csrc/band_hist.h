// The band histograms of the statistical route (R:scripts/statistical_analysis/statistical_analysis.py with
// fct_misc.get_pixel_values and fct_statistics.get_df_stats_groupby / get_df_stats_no_group, restated in
// proj_roadsurf_amd/band_stats.py) as a per-pixel rule.  Shared by band_hist_kernel (band_hist.hip) and the host restatement behind
// rs_host_band_hist (the same file's host half); DESIGN.md section 3.5 states it.
//
// For tile t the label instances are g = tile_first[t] .. tile_first[t + 1] - 1, the bands c < C, the values v < 256, and
//   hist[g][c][v] = the number of pixels (x, y), x < side, y < side, of tile t with
//     bit x % 8 of byte x / 8 of row y of canvas g set                  (the road's pixels on this tile),
//     not all C bands of the pixel 0                                    (the reference's nodata rule without a nodata value),
//     band c of the pixel == v.
// A pixel with some bands 0 and others not is counted and lands in bin 0 of its zero bands.  Every statistic the reference tabulates
// per road and band (min, max, median, mean, std, count) is an exact function of these counts.
//
// TABLES: tiles [n][side][side][C] uint8, interleaved; canvases [n_inst][side][(side + 7) / 8] bytes as canvas_raster_kernel writes
// them; hist [n_inst][C][256] uint32, compact by instance.  Integers only: counts add exactly over workgroups, tiles, batches and
// ranks in any order, so the bits do not depend on the run.  A count is at most side * side <= 2^20.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BH_HD __host__ __device__ __forceinline__
#else
#define BH_HD inline
#endif

#define BH_BINS 256
#define BH_MAX_SIDE 1024       // = CR_MAX_SIDE, what the canvases in front of this stage hold
#define BH_MAX_CHANNELS 4

// bytes of one canvas row / of one canvas
BH_HD int bh_row_bytes(int side) { return (side + 7) >> 3; }
BH_HD long long bh_canvas_bytes(int side) { return (long long)side * bh_row_bytes(side); }

// the nodata rule: is the pixel (its C interleaved bytes at px) one the statistics see?
BH_HD bool bh_has_data(const uint8_t* px, int C) {
  unsigned any = 0;
  for (int c = 0; c < C; ++c) any |= px[c];
  return any != 0;
}

// Row of canvas byte b without a division: magic = floor(2^40 / row_bytes) + 1 (bh_row_magic, formed once on the host).  With
// magic * row_bytes = 2^40 + e, 0 < e <= row_bytes <= 128, the product b * magic / 2^40 exceeds b / row_bytes by b * e / (row_bytes *
// 2^40) < 1 / row_bytes for every b < 2^33; a canvas has at most 2^17 bytes, so the floor is the quotient's and b * magic < 2^58.
BH_HD unsigned bh_row_of(unsigned b, unsigned long long magic) { return (unsigned)(((unsigned long long)b * magic) >> 40); }
inline unsigned long long bh_row_magic(int row_bytes) { return (1ull << 40) / (unsigned long long)row_bytes + 1ull; }
