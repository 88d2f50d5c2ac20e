// The area of (road label ∩ detection) on POLYGONS, as the reference's overlay takes it (R:scripts/road_segmentation/
// determine_class.py:97-120: round(area(label ∩ detection) / area(label), 2) on the vector labels and the RDP-simplified detection
// polygons), stated once for poly_overlap_kernel (poly_vote.hip) and the host restatement behind rs_host_polygon_overlaps (the host
// half of the same file).  DESIGN.md section 3.5 ("polygon geometry") states it.  Every translation unit that includes this header is
// compiled WITHOUT mul+add contraction; float64 throughout, the compiler's correctly rounded float64 division.
//
// THE RULE.  No topological clipping.  For a polygon P with rings r let role(r) = +1 for an exterior and -1 for a hole, orient(r) the
// sign of the ring's own shoelace sum.  Edge e = (start -> end) of ring r gets the sign s_e = role(r) * orient(r) * sgn(x_start - x_end)
// (0 for a vertical edge).  For every x the signed half lines below the edges over x sum to the indicator of P's column, whatever the
// stored orientation of the rings, so
//     area(P ∩ Q) = sum_{e in P} sum_{f in Q} s_e * s_f * integral over X_e ∩ X_f of min(y_e(x), y_f(x)) dx,
// X an edge's x-interval and y its line.  Since sum_e s_e [x in X_e] = 0 for every x, the double sum does not depend on the baseline the
// ordinates are measured from: ordinates may be negative, the baseline only sets the magnitudes that are rounded.
//
// OPERANDS.  Detection: one instance of the polygoniser's tables (include/rs_engine.h, RS_POLY_HDR): header = {flagged, polygons,
// rings, vertices, first polygon, first ring, first vertex, 0}, poly_ring_count, ring_len, xy int16 pairs; rings are closed (first ==
// last vertex, ring_len - 1 edges), the first ring of a polygon is its exterior and the rest are holes, an instance of several
// polygons is their sum.  Label: rings ring_first .. ring_last - 1 of the label tables (poly_off in doubles into polys, poly_len
// doubles, x0 y0 x1 y1 ... float64 tile pixels, the closing edge implied; a ring that repeats its first vertex only adds an edge of
// length 0).  EVERY LABEL RING IS AN EXTERIOR, and a label's rings are taken as simple and pairwise interior-disjoint, like the parts
// of a MultiPolygon: area(label) = sum over rings of |shoelace| / 2.  This differs from the pixel geometry (road_vote.h), which takes
// the UNION of a label's rings, and it is NOT CHECKED: overlapping rings count their overlap twice, a label with a hole is not modelled.
//
// TRANSLATION.  Both operands are translated by (ox, oy) = (floor(min x), floor(min y)) of the label's vertices before anything else:
// exact for the int16 detection vertices and (Sterbenz / small integers) harmless for the labels' doubles.  Label ordinates are then >= 0.
//
// ONE PAIR OF EDGES (po_pair).  Edges are stored left to right: xl < xr, yl, slope m = (yr - yl) / (xr - xl), sign s; y(x) = yl +
// (x - xl) * m.  With a = max(xl_e, xl_f), b = min(xr_e, xr_f): nothing unless a < b; w = b - a; ordinates ea, eb, fa, fb at the two
// ends, da = ea - fa, db = eb - fb, ma / mb the smaller computed ordinate at each end.  da, db of strictly opposite signs: the lines
// cross at tc = |da| / (|da| + |db|) (a sum of magnitudes: well conditioned), w1 = w * tc, w2 = w - w1, yc = ea + (eb - ea) * tc,
// integral = 0.5 * (w1 * (ma + yc) + w2 * (yc + mb)); otherwise integral = 0.5 * (w * (ma + mb)).  The term is (s_e * s_f) * integral.
//
// SUMMATION ORDER, per (label, detection).  The label's edge slots j = 0, 1, ... are its vertices in table order, ring after ring
// (slot j = the edge from that vertex to the next of its ring, the last to the first).  They are taken in chunks of PO_STAGE slots
// (one chunk unless the label has more vertices than that).  Within a chunk: the detection's rings in table order; edge k of a ring
// (k = 0 .. ring_len - 2) belongs to lane k % 64; a lane takes its edges in ascending (ring, k) order and for each forms
//     row = 0.0; for j ascending over the chunk's slots: row += po_pair(label edge j, detection edge);   acc[lane] += row;
// acc starting at 0.0.  The 64 lanes are summed by the fixed tree  for off = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l ^ off]
// (a butterfly: IEEE addition commutes, every lane ends with the same bits; the host forms acc[l] += acc[l + off] for l < off and
// reads acc[0]).  The chunks' results are added in ascending order, starting from the first chunk's own value.  No atomics.
//
// THE WEIGHT.  frac = rint(A / area(label) * 100.0) / 100.0 (numpy's round(., 2), half to even, as rv_frac); an A that rounding made
// negative, or not above zero, gives 0.  A pair whose bounding boxes do not overlap in a set of positive area (detection box from its
// own vertices, exact compares on the untranslated values) gives exactly 0 and never enters the sum; so does a flagged instance, an
// instance without polygons and a label of area 0.
//
// ERROR BOUND (po_bound).  u = 2^-53.  Sx, Sy: the spans of the common box of both operands after the translation, extended to hold
// the origin, so that |x| <= Sx, |y| <= Sy, every width w <= Sx and every |yr - yl| <= Sy.  E = the label's edge slots, F = the
// detection's edges.  First order in u:
//   ordinate: m carries 3u (two differences, one division), (x - xl) one u, the product one more: 5u of a value <= |yr - yl| <= Sy,
//     and the final sum u * Sy: an ordinate is within 6u Sy of the line; we carry delta = 12u Sy (the integer detection side is exact in
//     its differences, the label side is not).  da, db are within eta = 2 delta + u * 2 Sy = 26u Sy.
//   no crossing computed: ma, mb are within delta of the true minima; a true crossing the compare missed has an end difference <= eta
//     and costs <= 0.5 w eta; three roundings of a value <= w Sy.  Sum: (12 + 13 + 3) u w Sy = 28u w Sy.
//   crossing computed at tc' for a true tc: |tc' - tc| (|da| + |db|) <= 3 eta + 8u Sy = 86u Sy, the area between the two broken lines is
//     half of that times w: 43u w Sy; yc carries 3 delta + 5u Sy = 41u Sy under the weight w / 2: 21u w Sy; ma, mb: 6u w Sy; the
//     roundings of w1, w2, the sums and the products: 10u w Sy.  Sum: 80u w Sy.
//   So one term is within PO_C_PAIR * u * Sx * Sy of its value, PO_C_PAIR = 96 holding both cases and the second-order remainder, and
//   its magnitude is <= Sx * Sy.
//   the sums: a value passes through at most E additions into its row, one per row of its lane -- a lane owns at most F / 64 + 1 edges
//     of every ring, the rings are at most F / 3 -- and 6 levels of the tree, plus one addition per further chunk (counted with the +9
//     slack below for up to two chunks; a label of more chunks adds 1 each, E / PO_STAGE in all, which po_bound adds).  Every partial
//     sum is <= E * F * Sx * Sy in magnitude, so the additions cost <= u * depth * E * F * Sx * Sy.
//   po_bound(E, F, Sx, Sy) = u * Sx * Sy * E * F * (PO_C_PAIR + E + F / 64 + F / 3 + E / PO_STAGE + 9).
// The bound is on |computed A - area(P ∩ Q)| for operands that satisfy the assumptions above.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PO_HD __host__ __device__ __forceinline__
#else
#define PO_HD inline
#endif

#define PO_STAGE 512           // label edge slots per chunk (the kernel's LDS stage: PO_STAGE * 5 doubles)
#define PO_LANES 64
#define PO_HDR 8               // = RS_POLY_HDR
#define PO_C_PAIR 96.0

struct PoEdge {
  double xl, xr, yl, m, s;     // left to right; s = 0 and xl == xr for a vertical (or empty) edge
};

// the edge (x0, y0) -> (x1, y1) of a ring with role * orient = ro (+1 / -1 / 0), translated coordinates
PO_HD void po_edge(PoEdge* e, double x0, double y0, double x1, double y1, double ro) {
  if (x0 < x1) {
    e->xl = x0; e->xr = x1; e->yl = y0; e->m = (y1 - y0) / (x1 - x0); e->s = -ro;
  } else if (x1 < x0) {
    e->xl = x1; e->xr = x0; e->yl = y1; e->m = (y0 - y1) / (x0 - x1); e->s = ro;
  } else {
    e->xl = x0; e->xr = x0; e->yl = y0; e->m = 0.0; e->s = 0.0;
  }
}

// s_e * s_f * integral over X_e ∩ X_f of min(y_e, y_f)
PO_HD double po_pair(const PoEdge& e, const PoEdge& f) {
  const double a = e.xl > f.xl ? e.xl : f.xl, b = e.xr < f.xr ? e.xr : f.xr;
  if (!(a < b)) return 0.0;
  const double ea = e.yl + (a - e.xl) * e.m, eb = e.yl + (b - e.xl) * e.m;
  const double fa = f.yl + (a - f.xl) * f.m, fb = f.yl + (b - f.xl) * f.m;
  const double da = ea - fa, db = eb - fb;
  const double ma = da <= 0.0 ? ea : fa, mb = db <= 0.0 ? eb : fb;
  const double w = b - a;
  double v;
  if ((da < 0.0 && db > 0.0) || (da > 0.0 && db < 0.0)) {
    const double ada = fabs(da), adb = fabs(db);
    const double tc = ada / (ada + adb);
    const double w1 = w * tc, w2 = w - w1;
    const double yc = ea + (eb - ea) * tc;
    v = 0.5 * (w1 * (ma + yc) + w2 * (yc + mb));
  } else {
    v = 0.5 * (w * (ma + mb));
  }
  return (e.s * f.s) * v;
}

// np.round(A / area, 2) of two polygon areas, area > 0; nothing for an A that is not above zero
PO_HD double po_frac(double A, double area) {
  if (!(A > 0.0)) return 0.0;
  const double q = A / area;
  const double m = rint(q * 100.0);
  return m / 100.0;
}

// the shoelace sum of a label ring of n vertices (x0 y0 x1 y1 ...), translated by (ox, oy), vertices in order, the closing edge last
PO_HD double po_ring_shoelace(const double* ring, int n, double ox, double oy) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const int k = i + 1 < n ? i + 1 : 0;
    const double x0 = ring[2 * i] - ox, y0 = ring[2 * i + 1] - oy, x1 = ring[2 * k] - ox, y1 = ring[2 * k + 1] - oy;
    s += x0 * y1 - x1 * y0;
  }
  return s;
}

// What the walk needs of a label: its box (untranslated), the origin, the area and the number of edge slots.  Sequential, in table order.
struct PoLabel {
  double xmin, xmax, ymin, ymax, ox, oy, area;
  int slots;
};
PO_HD void po_label_scan(PoLabel* L, const double* polys, const int* poly_off, const int* poly_len, int ring_first, int ring_last) {
  L->xmin = L->ymin = 0.0; L->xmax = L->ymax = 0.0; L->ox = L->oy = 0.0; L->area = 0.0; L->slots = 0;
  bool any = false;
  for (int r = ring_first; r < ring_last; ++r) {
    const double* ring = polys + poly_off[r];
    const int n = poly_len[r] / 2;
    for (int i = 0; i < n; ++i) {
      const double x = ring[2 * i], y = ring[2 * i + 1];
      if (!any) { L->xmin = L->xmax = x; L->ymin = L->ymax = y; any = true; }
      if (x < L->xmin) L->xmin = x;
      if (x > L->xmax) L->xmax = x;
      if (y < L->ymin) L->ymin = y;
      if (y > L->ymax) L->ymax = y;
    }
    L->slots += n > 0 ? n : 0;
  }
  L->ox = floor(L->xmin); L->oy = floor(L->ymin);
  for (int r = ring_first; r < ring_last; ++r) L->area += fabs(po_ring_shoelace(polys + poly_off[r], poly_len[r] / 2, L->ox, L->oy)) * 0.5;
}

// slot i of label ring `ring` (n vertices) whose shoelace sum is sh: every label ring is an exterior
PO_HD void po_label_edge(PoEdge* e, const double* ring, int n, int i, double sh, double ox, double oy) {
  const int k = i + 1 < n ? i + 1 : 0;
  const double ro = sh > 0.0 ? 1.0 : (sh < 0.0 ? -1.0 : 0.0);
  po_edge(e, ring[2 * i] - ox, ring[2 * i + 1] - oy, ring[2 * k] - ox, ring[2 * k + 1] - oy, ro);
}

// one term of a detection ring's shoelace sum: exact in 64-bit integers for int16 vertices, so its sign does not depend on the order
PO_HD long long po_det_cross(const int16_t* xy, int v) {
  return (long long)xy[2 * v] * (long long)xy[2 * v + 3] - (long long)xy[2 * v + 2] * (long long)xy[2 * v + 1];
}
// edge k of a detection ring that starts at vertex v0: role = +1 exterior / -1 hole, sh = the ring's shoelace sum
PO_HD void po_det_edge(PoEdge* f, const int16_t* xy, int v0, int k, int role, long long sh, double ox, double oy) {
  const int v = v0 + k;
  const double ro = (double)(role * (sh > 0 ? 1 : (sh < 0 ? -1 : 0)));
  po_edge(f, (double)xy[2 * v] - ox, (double)xy[2 * v + 1] - oy, (double)xy[2 * v + 2] - ox, (double)xy[2 * v + 3] - oy, ro);
}

// do the boxes overlap in a set of positive area?  detection box in integers, label box as scanned
PO_HD bool po_boxes_meet(const PoLabel& L, int dxmin, int dxmax, int dymin, int dymax) {
  return (double)dxmin < L.xmax && (double)dxmax > L.xmin && (double)dymin < L.ymax && (double)dymax > L.ymin;
}

// the bound on |computed area - exact area| derived above; E, F >= 1 edge counts, Sx, Sy the spans
PO_HD double po_bound(int E, int F, double Sx, double Sy) {
  const double u = 1.1102230246251565e-16;   // 2^-53
  const double depth = PO_C_PAIR + (double)E + (double)F / 64.0 + (double)F / 3.0 + (double)E / (double)PO_STAGE + 9.0;
  return u * Sx * Sy * (double)E * (double)F * depth;
}
