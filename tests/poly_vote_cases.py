"""Hand-built batches for the polygon geometry of the road vote (csrc/poly_overlap.h), shared by tests/test_poly_votes_cpu.py and
tests/test_gpu_poly_votes.py: the smallest shapes that can go wrong.  Tiles are 32 and 64 px; detection vertices are integers (pixel
corners; the first ring of a polygon is its exterior), label vertices lie on a quarter-pixel grid.  A case is a dict: ``name``,
``side``, ``dets[tile][instance]`` = list of polygons = list of rings of (x, y), or ``None`` for an instance the polygoniser flagged;
``labels[tile][label]`` = list of rings of (x, y); ``det_scores`` / ``det_classes`` (n, slots).  ``tables(case)`` gives the batch dict of
``raster_vote.POLY_TABLE_KEYS``; ``exact(name)`` gives, per (tile, instance, label) pair, the exact area from tests/poly_overlap_ref.py
with the label's exact area, the edge counts, the spans and ``po_bound``.  Every case also exists with every ring reversed
(``name + "/rev"``): the stored orientation must not matter."""
import functools
from fractions import Fraction

import numpy as np

from tests import poly_overlap_ref as ref

Q = Fraction(1, 4)
U53 = 2.0 ** -53
PO_STAGE = 512
PO_C_PAIR = 96.0
CAP = 128


def po_bound(E, F, Sx, Sy):
    """csrc/poly_overlap.h, po_bound, restated (the C function is inline in a header, not an entry of the library)."""
    return U53 * Sx * Sy * E * F * (PO_C_PAIR + E + F / 64.0 + F / 3.0 + E / PO_STAGE + 9.0)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def comb(x0, y0, n_edges, low, top):
    """A rectilinear comb with integer vertices and exactly n_edges edges: a base from y0 up to `low`, teeth of width 1 every 2 px up to
    `top` (4 edges per tooth), and n_edges % 4 further vertices on the base's bottom edge (collinear: one edge more each)."""
    teeth, extra = n_edges // 4, n_edges % 4
    W = 2 * teeth - 1
    pts = [(x0, y0)] + [(x0 + 1 + i, y0) for i in range(extra)] + [(x0 + W, y0)]
    for i in range(teeth):
        xr = x0 + W - 2 * i
        pts += [(xr, top), (xr - 1, top)]
        if i + 1 < teeth:
            pts += [(xr - 1, low), (xr - 2, low)]
    assert len(pts) == n_edges
    return pts


def zigzag(x0, yb, n_edges, yt, step):
    """A road-like strip with exactly n_edges edges on the quarter-pixel grid: a flat bottom at yb and a top that alternates between yt
    and yt + 3/4 every `step` px."""
    m = n_edges - 2
    pts = [(x0, yb), (x0 + (m - 1) * step, yb)]
    for i in range(m):
        pts.append((x0 + (m - 1 - i) * step, yt + (3 * Q if i % 2 else 0)))
    assert len(pts) == n_edges
    return pts


L_SHAPE = [(4, 4), (20, 4), (20, 10), (10, 10), (10, 22), (4, 22)]            # non-convex: the notch is x > 10, y > 10


def _base_cases():
    c = []
    c.append(dict(name="rects", side=32,
                  dets=[[[[rect(4, 4, 20, 16)]], [[rect(10, 2, 14, 30)]]]],
                  labels=[[[rect(2 + Q, 6 + 2 * Q, 26 + 3 * Q, 10 + Q)], [rect(12 + 2 * Q, 1 + Q, 17 + Q, 29 + 3 * Q)]]]))
    c.append(dict(name="triangle_L", side=32,
                  dets=[[[[L_SHAPE]]]],
                  labels=[[[[(2 + Q, 2 + Q), (24 + 2 * Q, 6 + Q), (6 + 3 * Q, 26 + Q)]]]]))
    c.append(dict(name="hole", side=32,
                  dets=[[[[rect(2, 2, 30, 30), rect(10, 10, 22, 22)]]]],
                  labels=[[[rect(8 + Q, 12 + Q, 25 + 2 * Q, 17 + 3 * Q)],            # over the hole: only its two ends are covered
                           [rect(12 + Q, 12 + 2 * Q, 20 + Q, 20 + 3 * Q)]]]))        # inside the hole: nothing
    c.append(dict(name="two_polygons", side=32,
                  dets=[[[[rect(2, 4, 10, 20)], [rect(16, 8, 28, 24), rect(19, 12, 25, 18)]]]],
                  labels=[[[rect(1 + Q, 10 + Q, 30 + 2 * Q, 14 + 3 * Q)]]]))
    # coincident collinear edges (the label's left and bottom edges lie on the detection's), shared vertices ((4, 4)), vertical edges
    c.append(dict(name="coincident", side=32,
                  dets=[[[[rect(4, 4, 20, 20)]], [[rect(12, 4, 28, 12)]]]],
                  labels=[[[rect(4, 4, 12, 9)], [[(4, 12), (20, 12), (20, 20 + 2 * Q), (12, 16 + Q), (4, 20 + 2 * Q)]]]]))
    # the boxes meet, the polygons do not: the label sits in the notch of the L
    c.append(dict(name="boxes_only", side=32,
                  dets=[[[[L_SHAPE]]]],
                  labels=[[[rect(12 + Q, 12 + Q, 19 + Q, 21 + Q)], [[(11, 10 + 2 * Q), (19 + 2 * Q, 10 + 2 * Q), (11, 21 + 2 * Q)]]]]))
    c.append(dict(name="inside", side=32,
                  dets=[[[[rect(2, 2, 30, 30)]], [[rect(12, 12, 16, 15)]]]],
                  labels=[[[rect(8 + Q, 9 + Q, 20 + Q, 18 + 2 * Q)]]]))         # inside the first (1.0), the second inside it
    for n in (63, 64, 65):
        c.append(dict(name=f"rings_{n}", side=64,
                      dets=[[[[comb(1, 2, n, 5, 10)]]]],
                      labels=[[[zigzag(Q, 3 + Q, n, 7 + Q, 1)]]]))
    c.append(dict(name="rings_129", side=64,
                  dets=[[[[comb(0, 2, 129, 5, 10)]]]],
                  labels=[[[zigzag(Q, 3 + Q, 129, 7 + Q, 2 * Q)]]]))
    # four tiles: no label; no detection; 128 labels (rows of 16 x 8 boxes of 3 x 5 px, every one under one of two detections or neither);
    # a flagged instance between two ordinary ones
    many = [[rect(1 + 4 * i + Q, 1 + 7 * j + Q, 4 * i + 4, 7 * j + 6 + Q)] for j in range(8) for i in range(16)]
    c.append(dict(name="tiles", side=64,
                  dets=[[[[rect(2, 2, 10, 10)]]],
                        [],
                        [[[rect(0, 0, 30, 64)]], [[rect(20, 10, 64, 40), rect(30, 16, 50, 30)]]],
                        [[[rect(4, 4, 20, 16)]], None, [[rect(10, 2, 14, 30)]]]],
                  labels=[[],
                          [[rect(2 + Q, 2 + Q, 9 + Q, 5 + Q)]],
                          many,
                          [[rect(2 + Q, 6 + 2 * Q, 26 + 3 * Q, 10 + Q)]]]))
    return c


def _reversed(case):
    r = dict(case)
    r["name"] = case["name"] + "/rev"
    r["dets"] = [[None if inst is None else [[ring[::-1] for ring in poly] for poly in inst] for inst in tile] for tile in case["dets"]]
    r["labels"] = [[[ring[::-1] for ring in lab] for lab in tile] for tile in case["labels"]]
    return r


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for b in _base_cases():
        for c in (b, _reversed(b)):
            n = len(c["dets"])
            slots = max(1, max(len(t) for t in c["dets"]))
            rng = np.random.default_rng(len(out) + 11)
            c["det_scores"] = rng.uniform(0.05, 1.0, (n, slots)).astype(np.float32)
            c["det_classes"] = rng.integers(0, 2, (n, slots)).astype(np.int32)
            out.append(c)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c["name"] == name)


def tile_tables(tile):
    """``engine.PolygonTables`` of one tile's instances; ``None`` = a flagged instance: the flag and no rows."""
    from proj_roadsurf_amd.raster_vote import polygon_tables_from_lists
    t = polygon_tables_from_lists([[] if inst is None else [[list(r) + [r[0]] for r in poly] for poly in inst] for inst in tile])
    for i, inst in enumerate(tile):
        if inst is None:
            t.header[i, 0] = 1
    return t


def float_labels(c):
    return [[[np.array([float(v) for p in ring for v in p]) for ring in lab] for lab in tile] for tile in c["labels"]]


def tables(c):
    """The batch dict of ``raster_vote.POLY_TABLE_KEYS``."""
    from proj_roadsurf_amd.raster_vote import pack_label_pool, stack_polygon_tables
    return {**stack_polygon_tables([tile_tables(t) for t in c["dets"]]), **pack_label_pool(float_labels(c))}


@functools.lru_cache(maxsize=None)
def exact(name):
    """{(tile, instance, label): dict(A, area, E, F, Sx, Sy, bound, boxes_meet)} with A and area exact Fractions."""
    c = case(name)
    out = {}
    for t, (dets, labs) in enumerate(zip(c["dets"], c["labels"])):
        for g, lab in enumerate(labs):
            lx = [Fraction(p[0]) for r in lab for p in r]
            ly = [Fraction(p[1]) for r in lab for p in r]
            ox, oy = min(lx).__floor__(), min(ly).__floor__()
            area = ref.rings_area(lab)
            for d, inst in enumerate(dets):
                if inst is None or not inst:
                    continue
                rings = [r for poly in inst for r in poly]
                dx = [p[0] for r in rings for p in r]
                dy = [p[1] for r in rings for p in r]
                meet = min(dx) < max(lx) and max(dx) > min(lx) and min(dy) < max(ly) and max(dy) > min(ly)
                Sx = float(max(max(lx), max(dx), ox) - min(min(lx), min(dx), ox))
                Sy = float(max(max(ly), max(dy), oy) - min(min(ly), min(dy), oy))
                E, F = sum(len(r) for r in lab), sum(len(r) for r in rings)
                out[(t, d, g)] = dict(A=ref.intersection_area(lab, rings), area=area, E=E, F=F, Sx=Sx, Sy=Sy, bound=po_bound(E, F, Sx, Sy),
                                      boxes_meet=meet)
    return out


def exact_frac(A, area):
    """round(A / area, 2) half to even, exactly; the cases keep 100 A / area away from the half-integers."""
    q = A / area * 100
    lo = q.__floor__()
    r = q - lo
    m = lo if r < Fraction(1, 2) else (lo + 1 if r > Fraction(1, 2) else lo + (lo & 1))
    return float(Fraction(m, 100))
