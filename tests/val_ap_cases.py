"""Ground-truth polygon families for the full-canvas rasteriser tests (tests/test_val_ap_cpu.py, tests/test_gpu_val_ap.py): each returns
``instances`` -- instances[g] = list of polygons ([x0, y0, x1, y1, ...] float64, canvas pixels) -- for a square canvas of a given side.
Deterministic per (name, side, n, seed).  ``DEGENERATE`` names the two families whose masks are all foreground / all background by
construction; every other family must cover a share of the canvases strictly between 1 % and 99 % (checked by the tests), so that none
can pass on empty or full masks."""
import zlib

import numpy as np

FAMILIES = ("inside", "far", "grid", "repeated", "hole", "many", "full", "outside")
DEGENERATE = ("full", "outside")


def _star(rng, cx, cy, r_lo, r_hi, k):
    """A star-shaped ring of k vertices around (cx, cy), radii in [r_lo, r_hi], random phase."""
    a = np.sort(rng.uniform(0, 2 * np.pi, k)) + rng.uniform(0, 2 * np.pi)
    r = rng.uniform(r_lo, r_hi, k)
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).reshape(-1)


def _inside(rng, side):
    polys = []
    for _ in range(int(rng.integers(1, 4))):
        r = rng.uniform(0.15, 0.45) * side
        cx, cy = rng.uniform(r, max(side - r, r + 1e-3), 2)
        p = _star(rng, cx, cy, 0.4 * r, r, int(rng.integers(3, 44)))
        polys.append(np.clip(p, 0.0, float(side)))
    return polys


def _far(rng, side):
    """Vertices up to 1000 px outside the canvas, the ring still crossing it."""
    k = int(rng.integers(3, 20))
    p = _star(rng, rng.uniform(-0.5, 1.5) * side, rng.uniform(-0.5, 1.5) * side, 0.05 * side, 0.05 * side + 1000.0, k)
    return [p]


def _grid(rng, side):
    """Integer and half-grid vertices: axis-aligned boxes, 45 degree diamonds and rings with dx == dy edges (the x-major tie)."""
    h = lambda lo, hi: float(rng.integers(int(2 * lo), int(2 * hi) + 1)) / 2.0
    kind = int(rng.integers(3))
    x0, y0 = h(-side / 4 - 1, side / 2), h(-side / 4 - 1, side / 2)
    w, t = h(0.5, side * 0.75 + 1), h(0.5, side * 0.75 + 1)
    if kind == 0:
        return [np.array([x0, y0, x0 + w, y0, x0 + w, y0 + t, x0, y0 + t])]
    if kind == 1:
        cx, cy, r = x0 + w, y0 + w, w
        return [np.array([cx - r, cy, cx, cy - r, cx + r, cy, cx, cy + r])]
    # an octagon-like ring: axis-aligned runs joined by exact diagonals (dx == dy at scale 5 too: the coordinates are on the half grid)
    c = h(0.5, max(w, t) / 2 + 0.5)
    return [np.array([x0 + c, y0, x0 + c + w, y0, x0 + 2 * c + w, y0 + c, x0 + 2 * c + w, y0 + c + t, x0 + c + w, y0 + 2 * c + t,
                      x0 + c, y0 + 2 * c + t, x0, y0 + c + t, x0, y0 + c])]


def _repeated(rng, side):
    """Repeated vertices (the closing one included) and collinear points on the edges."""
    r = rng.uniform(0.2, 0.5) * side
    base = _star(rng, rng.uniform(0.3, 0.7) * side, rng.uniform(0.3, 0.7) * side, 0.5 * r, r, int(rng.integers(3, 12))).reshape(-1, 2)
    out = []
    for i in range(len(base)):
        a, b = base[i], base[(i + 1) % len(base)]
        out.append(a)
        if rng.random() < 0.5:
            out.append(a.copy())                          # the same vertex twice
        if rng.random() < 0.5:
            out.append(a + (b - a) * 0.5)                 # a point on the edge
    out.append(base[0].copy())                            # closed the COCO way: first == last
    return [np.concatenate(out)]


def _hole(rng, side):
    """An outer ring, a hole ring inside it (opposite orientation) and a second part: polygons of one instance are united."""
    cx, cy = rng.uniform(0.3, 0.7, 2) * side
    r = rng.uniform(0.3, 0.45) * side
    outer = _star(rng, cx, cy, 0.8 * r, r, 16)
    inner = _star(rng, cx, cy, 0.45 * r, 0.65 * r, 9).reshape(-1, 2)[::-1].reshape(-1)
    part = _star(rng, rng.uniform(0, 1) * side, rng.uniform(0, 1) * side, 0.03 * side, 0.1 * side, 5)
    return [outer, inner, part]


def _many(rng, side):
    r = rng.uniform(0.25, 0.5) * side
    return [_star(rng, rng.uniform(0.0, 1.0) * side, rng.uniform(0.0, 1.0) * side, 0.7 * r, r, int(rng.integers(300, 700)))]


def _full(rng, side):
    m = rng.uniform(1.0, 50.0)
    return [np.array([-m, -m, side + m, -m, side + m, side + m, -m, side + m])]


def _outside(rng, side):
    dx = side + rng.uniform(2.0, 500.0)
    return [_star(rng, dx + 0.3 * side, rng.uniform(-1, 2) * side, 0.1 * side, 0.3 * side, int(rng.integers(3, 12)))]


_MAKERS = {"inside": _inside, "far": _far, "grid": _grid, "repeated": _repeated, "hole": _hole, "many": _many, "full": _full, "outside": _outside}


def family(name: str, side: int, n: int, seed: int = 0):
    rng = np.random.default_rng([seed, side, zlib.crc32(name.encode())])
    return [_MAKERS[name](rng, side) for _ in range(n)]


def tables(instances):
    """The flat polygon tables of rs_op_mask_targets / rs_op_rasterize_canvas: (flat float64, poly_off int64, poly_len int32, inst_first int32)."""
    arrs = [np.asarray(p, np.float64).reshape(-1) for polys in instances for p in polys]
    lens = np.array([a.size for a in arrs] or [0], np.int32)
    off = np.zeros(max(len(arrs), 1), np.int64)
    if len(arrs) > 1:
        off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(1)
    first = np.zeros(len(instances) + 1, np.int32)
    first[1:] = np.cumsum([len(polys) for polys in instances])
    return flat, off, lens, first


_HOST = {}


def host_masks(name: str, side: int, n: int, seed: int = 0) -> np.ndarray:
    """(n, side, side) bool of rs_rasterize_polygons_within_box at box (0, 0, side, side): computed once per case and shared (read-only)."""
    key = (name, side, n, seed)
    if key not in _HOST:
        from proj_roadsurf_amd.train_targets import rasterize_polygons_within_box
        box = np.array([0.0, 0.0, side, side])
        m = np.stack([rasterize_polygons_within_box(p, box, side) for p in family(name, side, n, seed)])
        m.setflags(write=False)
        _HOST[key] = m
    return _HOST[key]


def unpack(packed: np.ndarray, side: int) -> np.ndarray:
    """(n, side, ceil(side / 8)) bytes in the rs_dets.masks layout -> (n, side, side) bool; the padding bits must be zero."""
    bits = np.unpackbits(packed, axis=-1, bitorder="little")
    assert not bits[:, :, side:].any(), "padding bits set"
    return bits[:, :, :side].astype(bool)
