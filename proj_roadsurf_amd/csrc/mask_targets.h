// Closed form of the mask head's training targets (vectorize.cpp: rs_rasterize_polygons_within_box + rle_fr_poly, i.e.
// detectron2's rasterize_polygons_within_box over pycocotools' rleFrPoly) without the walk along the 5x up-sampled boundary.
// Shared by mask_targets_kernel (train_kernels.hip) and host code that wants to state the same rules; DESIGN.md section 8 ("Mask targets on the device") derives them.
//
// rleFrPoly walks every edge point by point (u, v), keeps the steps between two consecutive points whose u differs and whose
// smaller u is c = 5m + 2 (the centre of column m at scale 5), and emits the point m * S + ceil(clamp((min v + .5) / 5 - .5)).
// Along one edge u is monotone and moves by at most one per step, and u does not change across the joint of two edges where it is
// positive, so each (edge, column) pair holds at most one such step and it can be located directly:
//   x-major (dx >= dy)   u(t) = xs + t:                    the step is t = c - xs, t + 1 when xs <= c and c + 1 <= xe
//   y-major (dx <  dy)   u(t) = (int)(xs + s * t + .5):    bisection on that very expression over [0, dy], at most 31 halvings
// All arithmetic is the host's, in fp64 and in the host's operand order; compile without mul+add contraction.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MT_HD __host__ __device__ __forceinline__
#else
#define MT_HD inline
#endif

#define MT_MAX_SIDE 28     // largest mask side the LDS counters of the kernel are sized for (RS_MASK_SIDE)
#define MT_MAX_DOUBLES (1 << 26)   // most doubles one polygon pool may hold: (edge, column) pairs are counted in 32 bits

struct MtBox {
  double x1, y1, ratio_w, ratio_h;
};

// box (x1, y1, x2, y2 as fp32, widened) -> offset and the two ratios of rasterize_polygons_within_box
MT_HD MtBox mt_box(float bx1, float by1, float bx2, float by2, int S) {
  MtBox b;
  b.x1 = (double)bx1; b.y1 = (double)by1;
  const double w = (double)bx2 - b.x1, h = (double)by2 - b.y1;
  b.ratio_h = S / (h < 0.1 ? 0.1 : h);          // std::max(h, 0.1)
  b.ratio_w = S / (w < 0.1 ? 0.1 : w);
  return b;
}

// one coordinate pair -> rleFrPoly's integer vertex at scale 5 ((int) truncates toward zero; negative values occur)
MT_HD void mt_vertex(const MtBox& b, double x, double y, int* X, int* Y) {
  double px = x - b.x1, py = y - b.y1;
  px *= b.ratio_w; py *= b.ratio_h;             // the host's ratio_h == ratio_w branch multiplies by the same two values
  *X = (int)(5.0 * px + .5);
  *Y = (int)(5.0 * py + .5);
}

// The point that edge (xs, ys) -> (xe, ye) emits for column m of an S x S mask: m * S + row in [m * S, m * S + S], or -1 for none.
MT_HD int mt_edge_point(int xs, int ys, int xe, int ye, int m, int S) {
  const int dx = xe > xs ? xe - xs : xs - xe, dy = ys > ye ? ys - ye : ye - ys;
  if (dx == 0) return -1;                       // u is constant along the edge (a repeated vertex included)
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
  const int c = 5 * m + 2;
  int vmin;
  if (dx >= dy) {                               // a tie is x-major
    if (!(xs <= c && c + 1 <= xe)) return -1;
    const double s = (double)(ye - ys) / dx;
    const int t = c - xs;
    const int v0 = (int)(ys + s * t + .5), v1 = (int)(ys + s * (t + 1) + .5);
    vmin = v0 < v1 ? v0 : v1;
  } else {
    if (xs < xe ? (c + 1 < xs || xe < c) : (c + 1 < xe || xs < c)) return -1;   // u stays within [min - 1, max + 1]: cheap reject
    const double s = (double)(xe - xs) / dy;
    const int u0 = (int)(xs + s * 0 + .5), u1 = (int)(xs + s * dy + .5);
    int lo = 0, hi = dy;                        // s > 0: u(lo) <= c < u(hi); s < 0: u(lo) > c >= u(hi)
    if (s > 0) {
      if (!(u0 <= c && u1 >= c + 1)) return -1;
      for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int)(xs + s * mid + .5) >= c + 1) hi = mid; else lo = mid;
      }
    } else {
      if (!(u0 >= c + 1 && u1 <= c)) return -1;
      for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int)(xs + s * mid + .5) <= c) hi = mid; else lo = mid;
      }
    }
    vmin = (hi - 1) + ys;                       // v(t) = t + ys: the smaller of the pair hi - 1, hi
  }
  double yd = (double)vmin;
  yd = (yd + .5) / 5.0 - .5;
  if (yd < 0) yd = 0; else if (yd > S) yd = S;
  int r = (int)yd;                              // ceil of a value in [0, S]
  if ((double)r < yd) ++r;
  return m * S + r;
}
