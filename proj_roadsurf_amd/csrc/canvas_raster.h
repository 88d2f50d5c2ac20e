// Per-column form of the closed-form rasteriser (mask_targets.h) for whole canvases: what canvas_raster_kernel (val_ap.hip) evaluates
// per (edge, column) pair, and what a host driver can state with the same functions.  DESIGN.md section 8 ("Validation AP on the
// device") says why columns are independent; tests/test_val_ap_cpu.py holds it against the host rasteriser.
//
// mask_targets.h numbers the points of a polygon column-major over the whole mask (m * S + row, row in [0, S]) and fills by the parity
// of the points at or before a cell.  A closed walk crosses the line between u = 5m + 2 and 5m + 3 an even number of times, so every
// column holds an even number of points and the parity carried into column m from the columns before it is zero -- the points that
// land on row S (= cell 0 of the next column) included, since they are counted with the column that emits them.  Hence column m is
// filled by the parity of ITS OWN points at rows <= the cell, and a point on row S toggles nothing inside the mask and is dropped.
#pragma once
#include "mask_targets.h"

#define CR_MAX_SIDE 1024   // largest canvas side (the polygoniser's max_side)

// floor(v / 5) for any sign
MT_HD int cr_floor5(int v) { return v >= 0 ? v / 5 : -((4 - v) / 5); }

// Columns m in [*m0, *m1], clipped to [lo, hi], that mt_edge_point can answer for an edge from xs to xe (scale-5 vertices): the
// x-major form needs min <= 5m + 2 < max, the y-major form rejects 5m + 3 < min and max < 5m + 2, so min - 1 <= 5m + 2 <= max covers
// both.  Empty when *m0 > *m1.
MT_HD void cr_edge_columns(int xs, int xe, int lo, int hi, int* m0, int* m1) {
  const int mn = xs < xe ? xs : xe, mx = xs < xe ? xe : xs;
  const int a = cr_floor5(mn - 3 + 4), b = cr_floor5(mx - 2);       // ceil((mn - 1 - 2) / 5), floor((mx - 2) / 5)
  *m0 = a > lo ? a : lo;
  *m1 = b < hi ? b : hi;
}

// Row in [0, S) of the point the edge emits for column m, or -1 (none, or a point on row S)
MT_HD int cr_edge_row(int xs, int ys, int xe, int ye, int m, int S) {
  const int pt = mt_edge_point(xs, ys, xe, ye, m, S);
  if (pt < 0) return -1;
  const int r = pt - m * S;
  return r < S ? r : -1;
}

// Inclusive prefix parity of the bits of one 32-bit word, bit 0 first; `carry` (0 / 1) is the parity of everything before the word
MT_HD uint32_t cr_prefix_parity(uint32_t x, uint32_t carry) {
  x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
  return carry ? ~x : x;
}
