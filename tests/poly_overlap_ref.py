"""An exact checker for the polygon overlaps of csrc/poly_overlap.h, in ``fractions.Fraction`` and by ANOTHER algorithm than the one
under test: slab decomposition.  The plane is cut at every vertex x of both operands and at every x where an edge of one crosses an
edge of the other; inside a slab no two edges cross, so each operand's column is a list of even-odd intervals between consecutive
edges (ordered at the slab's middle), the interval lists are intersected, and every piece is a trapezoid integrated exactly.

An operand is a list of rings, a ring a list of (x, y) (closed or not; exact rationals or values that ``Fraction`` takes exactly:
ints, floats, strings).  Membership is even-odd over all rings, which is the region of a polygon with holes, of several disjoint
polygons, and of a label whose rings are interior-disjoint.  Each operand's own rings must not cross each other.

The file also holds the rule under test in exact arithmetic (``edge_terms``: the double sum of poly_overlap.h per edge), which the
cases use to show that every edge matters, and the two pins of the checker: areas worked out by hand, and pixel counts.

HAND AREAS (``HAND``), each the intersection of two operands:
  unit squares offset by (1/2, 1/2)                         -> 1/2 * 1/2 = 1/4
  square (0,0)-(4,4) and the triangle (0,0), (4,0), (0,4)   -> the triangle: 8
  square (0,0)-(4,4) and the triangle (2,2), (6,2), (2,6)   -> the triangle cut to x, y <= 4: right isosceles legs 2 from (2,2)
                                                               = square 2x2: 4, the hypotenuse x + y = 8 passes through (4,4): 4
  square (0,0)-(6,6) with the hole (2,2)-(4,4), and the
  rectangle (1,1)-(5,3)                                     -> 4 * 2 - (hole part 2 x 1) = 6
  two diamonds |x| + |y| <= 2 centred (0,0) and (2,0)       -> the lens is the diamond |x - 1| + |y| <= 1: area 2
"""
from fractions import Fraction
from typing import List, Sequence, Tuple

Ring = Sequence[Tuple[object, object]]


def _F(v) -> Fraction:
    return v if isinstance(v, Fraction) else Fraction(v)


def ring_edges(ring: Ring) -> List[Tuple[Fraction, Fraction, Fraction, Fraction]]:
    """The edges (x0, y0, x1, y1) of a ring, the closing edge included when the ring is open; edges of length 0 dropped."""
    pts = [(_F(x), _F(y)) for x, y in ring]
    if len(pts) > 1 and pts[0] == pts[-1]:
        pts = pts[:-1]
    out = []
    for i, (x0, y0) in enumerate(pts):
        x1, y1 = pts[(i + 1) % len(pts)]
        if (x0, y0) != (x1, y1):
            out.append((x0, y0, x1, y1))
    return out


def shoelace(ring: Ring) -> Fraction:
    return sum((x0 * y1 - x1 * y0 for x0, y0, x1, y1 in ring_edges(ring)), Fraction(0))


def rings_area(rings: Sequence[Ring]) -> Fraction:
    """Sum of |shoelace| / 2 over the rings: the area of a label whose rings are simple and interior-disjoint."""
    return sum((abs(shoelace(r)) / 2 for r in rings), Fraction(0))


def _slanted(rings: Sequence[Ring]):
    """Non-vertical edges left to right: (xl, yl, xr, yr)."""
    out = []
    for r in rings:
        for x0, y0, x1, y1 in ring_edges(r):
            if x0 < x1:
                out.append((x0, y0, x1, y1))
            elif x1 < x0:
                out.append((x1, y1, x0, y0))
    return out


def _y_at(e, x: Fraction) -> Fraction:
    xl, yl, xr, yr = e[:4]
    return yl + (x - xl) * (yr - yl) / (xr - xl)


def _crossing_x(e, f):
    """x of the crossing of two slanted edges inside both x-ranges, or None (parallel or apart)."""
    me = (e[3] - e[1]) / (e[2] - e[0])
    mf = (f[3] - f[1]) / (f[2] - f[0])
    if me == mf:
        return None
    # e: y = e1 + (x - e0) me ; f: y = f1 + (x - f0) mf
    x = (f[1] - e[1] + e[0] * me - f[0] * mf) / (me - mf)
    lo, hi = max(e[0], f[0]), min(e[2], f[2])
    return x if lo < x < hi else None


def _intervals(edges, xa: Fraction, xb: Fraction, xm: Fraction):
    """Even-odd intervals (lower edge, upper edge) of the edges that span the slab."""
    span = [e for e in edges if e[0] <= xa and e[2] >= xb]
    span.sort(key=lambda e: (_y_at(e, xm), _y_at(e, xb) - _y_at(e, xa)))
    assert len(span) % 2 == 0, "an operand's rings are not closed"
    return [(span[i], span[i + 1]) for i in range(0, len(span), 2)]


def intersection_area(P: Sequence[Ring], Q: Sequence[Ring]) -> Fraction:
    """area(P ∩ Q), exactly."""
    ep, eq = _slanted(P), _slanted(Q)
    xs = {e[0] for e in ep + eq} | {e[2] for e in ep + eq}
    for e in ep:
        for f in eq:
            if e[2] <= f[0] or f[2] <= e[0]:
                continue
            x = _crossing_x(e, f)
            if x is not None:
                xs.add(x)
    xs = sorted(xs)
    total = Fraction(0)
    for xa, xb in zip(xs[:-1], xs[1:]):
        xm = (xa + xb) / 2
        ip, iq = _intervals(ep, xa, xb, xm), _intervals(eq, xa, xb, xm)
        for lp, up in ip:
            for lq, uq in iq:
                lo = lp if _y_at(lp, xm) >= _y_at(lq, xm) else lq
                hi = up if _y_at(up, xm) <= _y_at(uq, xm) else uq
                if _y_at(lo, xm) < _y_at(hi, xm):
                    total += ((_y_at(hi, xa) - _y_at(lo, xa)) + (_y_at(hi, xb) - _y_at(lo, xb))) / 2 * (xb - xa)
    return total


# ---------------------------------------------------------------------------------------------------- the rule under test, exactly
def signed_edges(rings: Sequence[Ring], roles: Sequence[int]):
    """Every edge of the rings as (xl, yl, xr, yr, s), s = role * orient * sgn(x_start - x_end) (csrc/poly_overlap.h); vertical edges
    keep s = 0 so that the list has one entry per edge."""
    out = []
    for ring, role in zip(rings, roles):
        sh = shoelace(ring)
        orient = (sh > 0) - (sh < 0)
        for x0, y0, x1, y1 in ring_edges(ring):
            if x0 < x1:
                out.append((x0, y0, x1, y1, -role * orient))
            elif x1 < x0:
                out.append((x1, y1, x0, y0, role * orient))
            else:
                out.append((x0, y0, x1, y1, 0))
    return out


def _pair_integral(e, f) -> Fraction:
    a, b = max(e[0], f[0]), min(e[2], f[2])
    if not a < b:
        return Fraction(0)
    ea, eb, fa, fb = _y_at(e, a), _y_at(e, b), _y_at(f, a), _y_at(f, b)
    da, db = ea - fa, eb - fb
    if da * db < 0:
        tc = abs(da) / (abs(da) + abs(db))
        xc = a + (b - a) * tc
        yc = _y_at(e, xc)
        return ((xc - a) * (min(ea, fa) + yc) + (b - xc) * (yc + min(eb, fb))) / 2
    return (b - a) * (min(ea, fa) + min(eb, fb)) / 2


def edge_terms(P_edges, Q_edges) -> Tuple[List[Fraction], List[Fraction]]:
    """Per edge of P and per edge of Q, the part of the double sum of poly_overlap.h that the edge carries: removing the edge changes the
    sum by that much, flipping its sign by twice that.  sum(terms of P) == sum(terms of Q) == the area."""
    tp, tq = [Fraction(0)] * len(P_edges), [Fraction(0)] * len(Q_edges)
    for i, e in enumerate(P_edges):
        if e[4] == 0:
            continue
        for j, f in enumerate(Q_edges):
            if f[4] == 0 or e[2] <= f[0] or f[2] <= e[0]:
                continue
            v = e[4] * f[4] * _pair_integral(e, f)
            tp[i] += v
            tq[j] += v
    return tp, tq


# ---------------------------------------------------------------------------------------------------- the pins
def _sq(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


HALF = Fraction(1, 2)
HAND = (
    ([_sq(0, 0, 1, 1)], [_sq(HALF, HALF, 1 + HALF, 1 + HALF)], Fraction(1, 4)),
    ([_sq(0, 0, 4, 4)], [[(0, 0), (4, 0), (0, 4)]], Fraction(8)),
    ([_sq(0, 0, 4, 4)], [[(2, 2), (6, 2), (2, 6)]], Fraction(4)),
    ([_sq(0, 0, 6, 6), _sq(2, 2, 4, 4)], [_sq(1, 1, 5, 3)], Fraction(6)),
    ([[(-2, 0), (0, -2), (2, 0), (0, 2)]], [[(0, 0), (2, -2), (4, 0), (2, 2)]], Fraction(2)),
)
