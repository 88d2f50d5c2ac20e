"""Plain-Python statement of the formulation the device polygoniser implements (csrc/polygonize.hip): a tracer
without the sequential "remove edges as you walk" state of oracle/host_tail_oracle.py, and Ramer-Douglas-Peucker with an integer
argmax.  tests/test_polygonize_cpu.py compares it with the oracle; the masks below are shared with tests/test_gpu_polygonize.py and
tests/test_gpu_polygonize_limits.py.

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
    c = m[1:-1, 1:-1]
    emits = c & ~(m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:])       # foreground with a background neighbour, visited row-major
    for y, x in zip(*(a.tolist() for a in np.nonzero(emits))):
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


# ------------------------------------------------------------------------------------------------ masks at the kernel's capacities
EDGE_CAP, RING_CAP, VERTEX_CAP, MAX_SIDE = 4096, 512, 4096, 1024       # csrc/polygonize.h; the GPU tests compare them with rs_polygonize_caps


def edge_count(mask: np.ndarray) -> int:
    """E: (foreground pixel, 4-neighbour that is background or outside the canvas) pairs."""
    m = np.pad(np.asarray(mask, bool), 1)
    c = m[1:-1, 1:-1]
    return int((c & ~m[:-2, 1:-1]).sum() + (c & ~m[2:, 1:-1]).sum() + (c & ~m[1:-1, :-2]).sum() + (c & ~m[1:-1, 2:]).sum())


def counts(mask: np.ndarray) -> Tuple[int, int, int]:
    """(E, R, V) of a mask by the formulation above: directed edges, rings of mask_to_polygons, closed ring lengths before simplification."""
    mask = np.asarray(mask, bool)
    polys = mask_to_polygons(mask)
    e = edge_count(mask)
    assert e == len(edges_of(mask))
    return e, sum(len(p) for p in polys), sum(len(r) for p in polys for r in p)


def over_a_cap(c: Tuple[int, int, int]) -> bool:
    """What the kernel must flag, from the counts alone."""
    return c[0] > EDGE_CAP or c[1] > RING_CAP or c[2] > VERTEX_CAP


def stripes_mask(extra: bool = False) -> np.ndarray:
    """63 x 64: rows 0, 2, .., 62 set in columns 0..62 -- 32 rectangles of 128 edges; ``extra`` adds pixel (0, 63)."""
    m = np.zeros((63, 64), bool)
    m[0::2, 0:63] = True
    if extra:
        m[0, 63] = True
    return m


def dots_mask(extra: bool = False) -> np.ndarray:
    """31 x 63 (33 x 63 with ``extra``): isolated pixels at even row and even column of rows 0..30 -- 512 rings; ``extra`` adds (32, 0)."""
    m = np.zeros((33 if extra else 31, 63), bool)
    m[0:31:2, 0::2] = True
    if extra:
        m[32, 0] = True
    return m


def vertex_mask(dots: int) -> np.ndarray:
    """72 x 152: nine diagonal bands two pixels wide (0 <= x - y - 4b <= 1: 4 * 72 + 1 vertices each), two empty columns, then a
    72 x 40 block of isolated pixels at (even row, odd column) filled row-major (5 vertices each)."""
    h, w = 72, 152
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for b in range(9):
        m |= (xx - yy - 4 * b >= 0) & (xx - yy - 4 * b <= 1)
    x0 = int(np.nonzero(m.any(axis=0))[0].max()) + 3
    assert x0 + 40 <= w and 0 <= dots <= 36 * 20
    for k in range(dots):
        m[2 * (k // 20), x0 + 1 + 2 * (k % 20)] = True
    return m


def full_canvas_mask(cleared: bool = False) -> np.ndarray:
    m = np.ones((MAX_SIDE, MAX_SIDE), bool)
    if cleared:
        m[500, 300] = False
    return m


def staircase_mask(n: int = 200) -> np.ndarray:
    yy, xx = np.mgrid[0:n, 0:n]
    return xx <= yy


def road_mask() -> np.ndarray:
    """A road three pixels wide across the whole 1024 x 1024 canvas: y = 100 + 0.23 x + 30 sin(x / 160)."""
    m = np.zeros((MAX_SIDE, MAX_SIDE), bool)
    x = np.arange(MAX_SIDE)
    y = np.floor(100.0 + 0.23 * x + 30.0 * np.sin(x / 160.0)).astype(int)
    for d in (-1, 0, 1):
        m[y + d, x] = True
    return m


def far_corner_mask() -> np.ndarray:
    m = np.zeros((MAX_SIDE, MAX_SIDE), bool)
    m[1000:1024, 1001:1024] = True
    m[1005:1010, 1005:1012] = False
    return m


# name -> (builder, (E, R, V)): the counts are asserted on the CPU (tests/test_polygonize_cpu.py); the GPU tests predict the flag from them
CAPACITY_MASKS = {
    "stripes": (stripes_mask, (4096, 32, 160)),
    "stripes_plus_pixel": (lambda: stripes_mask(True), (4098, 32, 160)),
    "dots": (dots_mask, (2048, 512, 2560)),
    "dots_plus_pixel": (lambda: dots_mask(True), (2052, 513, 2565)),
    "vertices_299": (lambda: vertex_mask(299), (3806, 308, 4096)),
    "vertices_300": (lambda: vertex_mask(300), (3810, 309, 4101)),
    "full_canvas": (full_canvas_mask, (4096, 1, 5)),
    "full_canvas_cleared_pixel": (lambda: full_canvas_mask(True), (4100, 2, 10)),
    "staircase_200": (staircase_mask, (800, 1, 403)),
    "road": (road_mask, (2530, 1, 957)),
    "far_corner_hole": (far_corner_mask, (118, 2, 10)),
}

# random 64 x 64 masks that straddle one cap with the other two counts under theirs: (density, seeds, cap straddled)
RANDOM_POPULATIONS = {"edges": (0.5, tuple(range(8)), 0), "rings": (0.35, tuple(range(8)), 1)}


def random_population(which: str) -> List[np.ndarray]:
    dens, seeds, _ = RANDOM_POPULATIONS[which]
    return [random_masks(1, 64, 64, dens, s)[0] for s in seeds]


# ------------------------------------------------------------------------------------------------ the engine's form of the call: crops
def pad_to(mask: np.ndarray, h: int, w: int, y0: int = 0, x0: int = 0) -> np.ndarray:
    """``mask`` placed at (y0, x0) of an empty h x w canvas."""
    m = np.zeros((h, w), bool)
    m[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]] = mask
    return m


def crop_bits(canvas: np.ndarray, rect) -> np.ndarray:
    """The pixels a rect [first byte column, first row, bytes per row, rows] covers, cut at the canvas width."""
    x0b, oy, wb, rows = (int(v) for v in rect)
    return np.asarray(canvas, bool)[oy:oy + rows, 8 * x0b:min(8 * (x0b + wb), canvas.shape[1])]


def crop_cases(h: int, w: int) -> Dict[str, Tuple[np.ndarray, Tuple[int, int, int, int], bool]]:
    """name -> (canvas, rect, the rect holds the whole mask) on a 24 x 40 or 45 x 45 canvas.  Every rect starts at a byte column > 0
    and a row > 0, so a kernel that forgets an offset gives other vertices, and the hole probes run at shifted coordinates."""
    assert (h, w) in ((24, 40), (45, 45))
    x0b, oy = (1, 3) if w == 40 else (2, 20)
    out: Dict[str, Tuple[np.ndarray, Tuple[int, int, int, int], bool]] = {}
    small = structured_masks(11, 13)
    for k in ("ring_with_hole", "nested_rings_island", "exteriors_after_hole"):
        out[k] = (pad_to(small[k], h, w, oy + 1, 8 * x0b + 2), (x0b, oy, 2, 12), True)
    # the same masks against the rect's first row and column: vertices on the rect's own border
    out["nested_at_rect_origin"] = (pad_to(small["nested_rings_island"], h, w, oy, 8 * x0b), (x0b, oy, 2, 12), True)
    # foreground of a random canvas cut by the rect on all four sides
    m = random_masks(1, h, w, 0.6, 11 + w)[0]
    rect = (x0b, oy, 2, 10)
    y1, xa, xb = oy + 10, 8 * x0b, 8 * x0b + 16
    m[oy - 1:oy + 1, xa + 3:xa + 6] = True; m[y1 - 1:y1 + 1, xa + 9:xa + 12] = True          # across the first and the last row
    m[oy + 4:oy + 6, xa - 1:xa + 1] = True; m[oy + 6:oy + 8, xb - 1:xb + 1] = True          # across the first and the last column
    out["cut_on_four_sides"] = (m, rect, False)
    if w == 45:
        # the rect's last byte crosses the canvas width: bytes 3..5 = columns 24..47, of which 24..44 exist
        m = np.zeros((h, w), bool)
        m[5:30, 38:45] = True; m[10:20, 40:43] = False; m[12, 41] = True; m[35, 44] = True; m[33:38, 26:30] = True
        out["last_byte_partial"] = (m, (3, 2, 3, 40), True)
    return out
