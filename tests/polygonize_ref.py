"""Plain-Python statement of the formulation the device polygoniser implements (csrc/polygonize.hip): a tracer
without the sequential "remove edges as you walk" state of oracle/host_tail_oracle.py, and Ramer-Douglas-Peucker with an integer
argmax.  tests/test_polygonize_cpu.py compares it with the oracle; the masks below are shared with tests/test_gpu_polygonize.py.

  1 edges      every foreground pixel, row-major, emits top (E), right (S), bottom (W), left (N) edges, foreground on the right;
               emission index t = 4 * (y * w + x) + k.  A vertex's rank is the smaller t of its (at most two) outgoing edges, an
               edge's key (rank of its start vertex, 0 if it is that first edge else 1).
  2 successor  of edge (v, d): at v' = v + D[d] the first of (d+1, d, d+3) mod 4 that v' has, among ALL its edges (static).
  3 rings      cycles of the successor; a ring starts at its edge of smallest key (found by pointer doubling, as the kernel does);
               rings are ordered by that key.
  4 vertices   start vertices of the edges whose direction differs from their predecessor's, in walk order from the start edge.
  5 area       shoelace on integers.
  6 holes      probe point in doubled integers, crossing test on vertical edges, smallest containing exterior, first on a tie.
  7 RDP        rings reversed (start vertex kept); integer numerator for the argmax (first maximum), float64 only against epsilon.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)


def edges_of(mask: np.ndarray) -> List[Tuple[int, int, int]]:
    """(x, y, d) of every directed edge in emission order."""
    h, w = mask.shape
    m = np.zeros((h + 2, w + 2), bool)
    m[1:-1, 1:-1] = mask.astype(bool)
    out = []
    for y in range(h):
        for x in range(w):
            if not m[y + 1, x + 1]:
                continue
            if not m[y, x + 1]:
                out.append((x, y, 0))
            if not m[y + 1, x + 2]:
                out.append((x + 1, y, 1))
            if not m[y + 2, x + 1]:
                out.append((x + 1, y + 1, 2))
            if not m[y + 1, x]:
                out.append((x, y + 1, 3))
    return out


def successor(edges: List[Tuple[int, int, int]]) -> List[int]:
    index = {e: i for i, e in enumerate(edges)}
    succ = []
    for x, y, d in edges:
        nx, ny = x + DX[d], y + DY[d]
        for c in ((d + 1) % 4, d, (d + 3) % 4):
            j = index.get((nx, ny, c))
            if j is not None:
                succ.append(j)
                break
        else:
            raise AssertionError("an edge without a successor")
    return succ


def edge_keys(edges: List[Tuple[int, int, int]]) -> List[int]:
    """2 * (index of the first-emitted edge at the start vertex) + slot: the order of (vertex rank, slot)."""
    first: Dict[Tuple[int, int], int] = {}
    keys = []
    for i, (x, y, _) in enumerate(edges):
        if (x, y) in first:
            keys.append(2 * first[(x, y)] + 1)
        else:
            first[(x, y)] = i
            keys.append(2 * i)
    return keys


def cycle_minimum(succ: List[int], keys: List[int]) -> List[int]:
    """Smallest key of every edge's cycle by pointer doubling: ceil(log2 E) rounds."""
    n = len(succ)
    nxt, mn = list(succ), list(keys)
    rounds = max(1, math.ceil(math.log2(max(n, 2))))
    for _ in range(rounds):
        mn2 = [min(mn[e], mn[nxt[e]]) for e in range(n)]
        nxt = [nxt[nxt[e]] for e in range(n)]
        mn = mn2
    return mn


def trace_rings(mask: np.ndarray) -> List[List[Tuple[int, int]]]:
    """Closed rings (integer vertices) in the oracle's discovery order, walking direction and start vertices."""
    edges = edges_of(mask)
    if not edges:
        return []
    succ = successor(edges)
    assert sorted(succ) == list(range(len(edges))), "the successor is not a bijection"
    keys = edge_keys(edges)
    mn = cycle_minimum(succ, keys)
    pred = [0] * len(edges)
    for e, s in enumerate(succ):
        pred[s] = e
    starts = sorted((keys[e], e) for e in range(len(edges)) if keys[e] == mn[e])
    rings = []
    for _, s in starts:
        ring = []
        e = s
        while True:
            if edges[e][2] != edges[pred[e]][2]:
                ring.append((edges[e][0], edges[e][1]))
            e = succ[e]
            if e == s:
                break
        ring.append(ring[0])
        rings.append(ring)
    return rings


def area2(ring) -> int:
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]))


def mask_to_polygons(mask: np.ndarray) -> List[List[List[Tuple[int, int]]]]:
    rings = trace_rings(np.asarray(mask))
    a2 = [area2(r) for r in rings]
    ext = [i for i, a in enumerate(a2) if a > 0]
    polys = {i: [i] for i in ext}
    for i, a in enumerate(a2):
        if a >= 0:
            continue
        (x0, y0), (x1, y1) = rings[i][0], rings[i][1]
        dx, dy = x1 - x0, y1 - y0
        px2 = x0 + x1 + (dy > 0) - (dy < 0)          # doubled coordinates of the probe point
        py2 = y0 + y1 - (dx > 0) + (dx < 0)
        best = None
        for x in ext:
            inside = False
            for (xa, ya), (xb, yb) in zip(rings[x][:-1], rings[x][1:]):
                if (2 * ya > py2) != (2 * yb > py2) and 2 * xa > px2:
                    inside = not inside
            if inside and (best is None or a2[x] < a2[best]):
                best = x
        if best is not None:
            polys[best].append(i)
    return [[list(reversed(rings[r])) for r in polys[x]] for x in ext]


def rdp(points, epsilon: float):
    """Ramer-Douglas-Peucker on integer points with the argmax on the integer numerator (first maximum)."""
    n = len(points)
    if n < 3 or epsilon <= 0:
        return list(points)
    keep = [False] * n
    keep[0] = keep[-1] = True
    stack = [(0, n - 1)]
    while stack:
        i0, i1 = stack.pop()
        if i1 <= i0 + 1:
            continue
        ax, ay = points[i0]
        sx, sy = points[i1][0] - ax, points[i1][1] - ay
        degenerate = sx == 0 and sy == 0
        best, bk = -1, -1
        for k in range(i0 + 1, i1):
            qx, qy = points[k][0] - ax, points[k][1] - ay
            v = qx * qx + qy * qy if degenerate else abs(sx * qy - sy * qx)
            if v > best:
                best, bk = v, k
        dist = math.sqrt(float(best)) if degenerate else float(best) / math.sqrt(float(sx * sx + sy * sy))
        if dist > epsilon:
            keep[bk] = True
            stack.append((i0, bk))
            stack.append((bk, i1))
    return [p for p, k in zip(points, keep) if k]


def polygons(mask: np.ndarray, epsilon: float):
    """What the device returns for one mask: polygons of rings of integer vertices, simplified."""
    out = []
    for poly in mask_to_polygons(mask):
        rings = []
        for r in poly:
            rr = rdp(r, epsilon) if epsilon > 0 else list(r)
            rings.append(rr if len(rr) >= 4 else list(r))
        out.append(rings)
    return out


# ------------------------------------------------------------------------------------------------ masks shared by the tests
def structured_masks(h: int, w: int) -> Dict[str, np.ndarray]:
    """The structured masks of the device tests on an h x w canvas (h >= 11, w >= 13)."""
    z = lambda: np.zeros((h, w), bool)
    out: Dict[str, np.ndarray] = {}
    out["empty"] = z()
    m = z(); m[0, 0] = True; out["pixel_first"] = m
    m = z(); m[h - 1, w - 1] = True; out["pixel_last"] = m
    m = z(); m[:, :] = True; out["full"] = m
    m = z(); m[3, :] = True; out["row"] = m
    m = z(); m[:, w - 2] = True; out["column"] = m
    m = z(); m[2, 2] = m[3, 3] = True; out["diag_down"] = m
    m = z(); m[2, 3] = m[3, 2] = True; out["diag_up"] = m
    m = z(); yy, xx = np.mgrid[0:8, 0:8]; m[1:9, 2:10] = (yy + xx) % 2 == 0; out["checkerboard8"] = m
    m = z(); m[1:8, 1:9] = True; m[3:6, 3:7] = False; out["ring_with_hole"] = m
    m = z(); m[0:11, 0:11] = True; m[1:10, 1:10] = False; m[2:9, 2:9] = True; m[3:8, 3:8] = False; m[4:7, 4:7] = True; m[5, 5] = False
    out["nested_rings_island"] = m
    # a ring whose hole is met first, then two separate regions whose exteriors are discovered after that hole
    m = z(); m[0:5, 0:7] = True; m[1:4, 1:6] = False; m[2, 3] = True; m[7:10, 1:4] = True; m[6:10, 8:12] = True; m[7:9, 9:11] = False
    out["exteriors_after_hole"] = m
    m = z(); m[1:9, 2:4] = True; m[7:9, 2:9] = True; out["L"] = m
    m = z(); m[1:9, 2:4] = True; m[1:9, 8:10] = True; m[7:9, 2:10] = True; out["U"] = m
    return out


def staircase_masks(h: int, w: int) -> Dict[str, np.ndarray]:
    """Unit staircases: every corner lies 1 / sqrt(2) from the diagonal chord, where the rounded fp64 quotient decides."""
    out: Dict[str, np.ndarray] = {}
    n = min(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    out["stairs_lower"] = (xx <= yy) & (yy < n)
    out["stairs_upper"] = (xx >= yy) & (xx < n)
    out["stairs_band"] = (np.abs(xx - yy) <= 1) & (xx < n) & (yy < n)
    out["stairs_anti"] = (xx + yy >= n - 1) & (xx < n) & (yy < n)
    return out


def random_masks(n: int, h: int, w: int, density: float, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((n, h, w)) < density


def pack(masks: np.ndarray) -> np.ndarray:
    """(n, h, w) bool -> (n, h, ceil(w/8)) uint8, the engine's layout (bit b of a byte = pixel 8 * byte + b)."""
    return np.packbits(np.asarray(masks, bool), axis=2, bitorder="little")
