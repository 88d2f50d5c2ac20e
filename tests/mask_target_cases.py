"""Polygon / box families for the mask-target rasteriser tests (tests/test_gpu_mask_targets.py): each returns
(instances, entry_instance, boxes) as ``train_targets.rasterize_entries`` takes them -- instances[g] = list of flat
[x0,y0,x1,y1,...] float64 polygons, entry e = instance entry_instance[e] inside boxes[e] (float32 x1,y1,x2,y2)."""
import numpy as np

FAMILIES = ("inside", "far", "grid", "integer", "repeated", "union", "long")
# the families whose scaled polygons stay small enough for the point-by-point Python oracle
ORACLE_FAMILIES = ("inside", "grid", "integer", "repeated", "union")


def _ring(rng, cx, cy, rx, ry, k):
    th = np.sort(rng.uniform(0, 2 * np.pi, k))
    r = rng.uniform(0.4, 1.0, k)
    return np.stack([cx + rx * r * np.cos(th), cy + ry * r * np.sin(th)], 1).reshape(-1)


def _unit_ratio_box(rng):
    """A box 28 x 28 with integer corners: both ratios are exactly 1, so scaled vertices are vertex minus corner."""
    x1, y1 = (float(v) for v in rng.integers(0, 200, 2) * rng.integers(0, 2))        # half of them at the origin: vertices exactly on the grid
    return np.array([x1, y1, x1 + 28.0, y1 + 28.0], np.float32)


def family(name: str, n_entries: int, seed: int = 0):
    rng = np.random.default_rng(seed + 1000 * FAMILIES.index(name))
    instances, boxes = [], []
    for _ in range(n_entries):
        if name == "inside":                 # polygons inside (and a little around) boxes of ordinary sizes
            w, h = rng.uniform(4, 200, 2)
            x1, y1 = rng.uniform(0, 300, 2)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            k = int(rng.integers(3, 9))
            polys = [_ring(rng, x1 + w * rng.uniform(0.2, 0.8), y1 + h * rng.uniform(0.2, 0.8), w * rng.uniform(0.2, 0.7), h * rng.uniform(0.2, 0.7), k)]
        elif name == "far":                  # instances reaching +-1000 px around boxes 0.05 .. 3 px wide: max(., 0.1) and large scaled coordinates
            w, h = rng.uniform(0.05, 3.0, 2)
            x1, y1 = rng.uniform(100, 200, 2)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            k = int(rng.integers(3, 7))
            pts = np.stack([x1 + rng.uniform(-1000, 1000, k), y1 + rng.uniform(-1000, 1000, k)], 1)
            pts[rng.integers(0, k)] = [x1 + w * rng.uniform(0, 1), y1 + h * rng.uniform(0, 1)]     # one vertex inside the box
            polys = [pts.reshape(-1)]
        elif name == "grid":                 # scaled vertices on multiples of 0.2 (the 5x grid) and +-0.1 of them (its half steps)
            box = _unit_ratio_box(rng)
            k = int(rng.integers(3, 9))
            g = rng.integers(-20, 160, (k, 2)) * 0.2 + rng.integers(-1, 2, (k, 2)) * 0.1
            polys = [(g + box[:2].astype(np.float64)).reshape(-1)]
        elif name == "integer":              # integer vertices: axis-aligned and 45 degree edges, the dx == dy tie
            box = _unit_ratio_box(rng)
            k = int(rng.integers(3, 9))
            p = [rng.integers(-4, 33, 2)]
            for _ in range(k - 1):
                d = int(rng.integers(1, 12))
                step = [(d, 0), (-d, 0), (0, d), (0, -d), (d, d), (-d, d), (d, -d), (-d, -d)][int(rng.integers(0, 8))]
                p.append(p[-1] + np.array(step))
            polys = [(np.array(p, np.float64) + box[:2].astype(np.float64)).reshape(-1)]
        elif name == "repeated":             # repeated consecutive vertices and collinear triples
            w, h = rng.uniform(10, 60, 2)
            x1, y1 = rng.uniform(0, 100, 2)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            base = _ring(rng, x1 + w / 2, y1 + h / 2, w * 0.6, h * 0.6, int(rng.integers(3, 7))).reshape(-1, 2)
            out = []
            for i, v in enumerate(base):
                out.append(v)
                r = int(rng.integers(0, 3))
                if r == 0:
                    out.append(v.copy())                                   # the same vertex twice
                elif r == 1:
                    out.append((v + base[(i + 1) % len(base)]) / 2)       # a point on the edge to the next vertex
            polys = [np.array(out).reshape(-1)]
        elif name == "union":                # 2..3 polygons per instance, one of them a hole ring (reversed, inside the first)
            w, h = rng.uniform(10, 120, 2)
            x1, y1 = rng.uniform(0, 200, 2)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            cx, cy = x1 + w / 2, y1 + h / 2
            outer = _ring(rng, cx, cy, w * 0.6, h * 0.6, int(rng.integers(4, 9)))
            hole = _ring(rng, cx, cy, w * 0.15, h * 0.15, int(rng.integers(3, 7))).reshape(-1, 2)[::-1].reshape(-1)
            polys = [outer, hole]
            if rng.integers(0, 2):
                polys.append(_ring(rng, x1 + w * rng.uniform(0, 1), y1 + h * rng.uniform(0, 1), w * 0.3, h * 0.3, int(rng.integers(3, 7))))
        elif name == "long":                 # several hundred vertices
            w, h = rng.uniform(20, 150, 2)
            x1, y1 = rng.uniform(0, 200, 2)
            box = np.array([x1, y1, x1 + w, y1 + h], np.float32)
            polys = [_ring(rng, x1 + w / 2, y1 + h / 2, w * 0.7, h * 0.7, int(rng.integers(300, 700)))]
        else:
            raise ValueError(name)
        instances.append([np.ascontiguousarray(p, np.float64) for p in polys])
        boxes.append(box)
    # entry e -> instance e, but walk them in a shuffled order so that entry and instance indices differ
    order = rng.permutation(n_entries).astype(np.int32)
    bx = np.stack([boxes[g] for g in order]).astype(np.float32) if n_entries else np.zeros((0, 4), np.float32)
    return instances, order, bx


def mixed(n_entries: int, seed: int = 0):
    """n_entries entries drawn in turn from the cheap families (entry-count sweeps)."""
    parts = [family(f, (n_entries + len(ORACLE_FAMILIES) - 1 - i) // len(ORACLE_FAMILIES), seed + 7) for i, f in enumerate(ORACLE_FAMILIES)]
    instances, ent, boxes = [], [], []
    for inst, order, bx in parts:
        ent.extend(int(o) + len(instances) for o in order)
        instances.extend(inst)
        boxes.extend(bx)
    assert len(ent) == n_entries
    return instances, np.array(ent, np.int32), (np.stack(boxes).astype(np.float32) if boxes else np.zeros((0, 4), np.float32))
