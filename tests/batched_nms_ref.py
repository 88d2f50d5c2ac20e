"""torchvision's batched_nms size rule, the way the kernels compute it, as the reference of the batched_nms tests, and the
fixtures that tell the rule's arithmetic from per-category arithmetic.

The kernels keep one workgroup per (image, category): category g of an image that takes the rule runs its NMS on
``boxes + fl(g * fl(max_coordinate + 1))``.  torchvision runs ONE NMS over the shifted boxes of all categories.  The two are
the same statement because shifted boxes of different categories never intersect; ``rule_keep`` is the per-category form
in NumPy and ``oracle_keep`` the oracle's (``oracle.maskrcnn_oracle.batched_nms``); tests/test_batched_nms_cpu.py holds
them equal, and the GPU tests then use ``rule_keep``."""
import numpy as np
import torch

from oracle import maskrcnn_oracle as O
from tests import util as U

_F32 = np.float32
RULE_MAX_BOXES = 1000          # boxes.numel() > 4000 is false up to 1000 boxes


def rule_decision(boxes, valid, counts):
    """(taken, unit, total) of ONE image: boxes [G][cap][4], valid [G][cap] (or None), counts [G].  total = valid entries of
    all categories; taken = 1 <= total <= 1000; unit = fl(max coordinate of those boxes + 1) in fp32, 0 where not taken."""
    G = len(counts)
    sel = [boxes[g, :counts[g]][valid[g, :counts[g]].astype(bool)] if valid is not None else boxes[g, :counts[g]] for g in range(G)]
    total = int(sum(len(s) for s in sel))
    if total < 1 or total > RULE_MAX_BOXES:
        return False, _F32(0), total
    mx = max(_F32(s.max()) for s in sel if len(s))
    return True, _F32(_F32(mx) + _F32(1)), total


def category_keep(boxes, valid, counts, t, unit=None):
    """Keep flags [G][cap] of ONE image from one NMS per category; ``unit`` given: on the coordinates shifted by
    fl(g * unit) -- the product rounded on its own, then one fp32 add per coordinate --, else on the boxes as they are."""
    G, cap = boxes.shape[:2]
    keep = np.zeros((G, cap), bool)
    for g in range(G):
        c = int(counts[g])
        v = valid[g, :c].astype(bool) if valid is not None else np.ones(c, bool)
        b = boxes[g, :c].astype(np.float32)
        if unit is not None:
            off = _F32(_F32(g) * _F32(unit))
            b = (b + off).astype(np.float32)
        keep[g, np.nonzero(v)[0][O.nms_sorted_np(b[v], t)]] = True
    return keep


def rule_keep(boxes, valid, counts, t):
    """The size rule on ONE image, per category: (keep [G][cap], taken, unit, total)."""
    taken, unit, total = rule_decision(boxes, valid, counts)
    return category_keep(boxes, valid, counts, t, unit if taken else None), taken, unit, total


def oracle_keep(boxes, valid, counts, t, coordinate_trick):
    """Keep flags [G][cap] of ONE image from ``oracle.batched_nms`` over its valid boxes, category = segment index.  Entry i of a
    segment outranks entry i + 1 (the segments are in priority order); across categories the scores interleave."""
    G, cap = boxes.shape[:2]
    bs, ss, ids, where = [], [], [], []
    for g in range(G):
        c = int(counts[g])
        v = np.nonzero(valid[g, :c])[0] if valid is not None else np.arange(c)
        bs.append(boxes[g, v])
        ss.append((1.0 - (v + 0.5 * g / max(G, 1)) / (cap + 1.0)).astype(np.float32))     # descending in the entry, distinct across categories
        ids.append(np.full(len(v), g, np.int64))
        where += [(g, int(i)) for i in v]
    keep = np.zeros((G, cap), bool)
    if not where:
        return keep
    kept = O.batched_nms(torch.from_numpy(np.concatenate(bs).astype(np.float32)), torch.from_numpy(np.concatenate(ss)),
                         torch.from_numpy(np.concatenate(ids)), t, coordinate_trick=coordinate_trick)
    for j in kept.tolist():
        keep[where[j]] = True
    return keep


# ------------------------------------------------------------------ fixtures
def threshold_pairs(rng, n_pairs, t, extent=512.0):
    """n_pairs pairs (A, B), A ahead of B: B is A moved right by w (1 - t) / (1 + t) * (1 + u), u uniform in +-3e-7, so that the
    pair's IoU (w - d) / (w + d) sits at t and its side of t depends on how the coordinates round.  [2 * n_pairs][4]."""
    w = rng.uniform(20.0, 120.0, n_pairs)
    h = rng.uniform(20.0, 120.0, n_pairs)
    x1 = rng.uniform(0.0, extent - 1.0, n_pairs)
    y1 = rng.uniform(0.0, extent - 1.0, n_pairs)
    d = w * (1.0 - t) / (1.0 + t) * (1.0 + rng.uniform(-3e-7, 3e-7, n_pairs))
    A = np.stack([x1, y1, x1 + w, y1 + h], 1)
    B = np.stack([x1 + d, y1, x1 + d + w, y1 + h], 1)
    return np.stack([A, B], 1).reshape(-1, 4).astype(np.float32)


def make_image(rng, G, cap, t, per_segment, invalid=0, edge_pairs=True, touch_border=True):
    """One image of G categories: per_segment[g] entries in category g.  A populated category starts with the edge pairs of
    tests/util.py nms_edge_pairs(t) (where they fit), then near-threshold pairs; `invalid` entries per populated category are
    marked invalid (they count for nothing).  touch_border: one box from coordinate 0 and one up to the image's largest
    coordinate, in the last populated category."""
    boxes = np.zeros((G, cap, 4), np.float32)
    valid = np.ones((G, cap), np.uint8)
    counts = np.zeros(G, np.int32)
    edges = U.nms_edge_pairs(t)[0] if edge_pairs else np.zeros((0, 4), np.float32)
    for g in range(G):
        c = int(per_segment[g])
        counts[g] = c
        if c == 0:
            continue
        b = threshold_pairs(rng, (c + 1) // 2, t)[:c]
        if c >= len(edges) + 8:
            b[:len(edges)] = edges
        boxes[g, :c] = b
        if invalid and c > invalid:
            bad = rng.choice(c, invalid, replace=False)
            valid[g, bad] = 0
    pop = [g for g in range(G) if counts[g] >= 4]
    if touch_border and pop:
        g = pop[-1]
        c = int(counts[g])
        mx = max(float(boxes[q, :counts[q]].max()) for q in range(G) if counts[q])
        boxes[g, c - 2] = [0.0, 0.0, 37.5, 41.25]
        boxes[g, c - 1] = [mx - 50.0, mx - 60.0, mx, mx]
        valid[g, c - 2:c] = 1
    return boxes, valid, counts


def spread(total, segments, G):
    """total entries over the listed segments of G (as evenly as integers allow), zeros elsewhere."""
    per = np.zeros(G, np.int64)
    for k, g in enumerate(segments):
        per[g] = total // len(segments) + (1 if k < total % len(segments) else 0)
    return per


def operator_fixture(G, cap, t, seed, kinds):
    """Images of one rs_op_batched_nms call, G category slots each.  kinds: list of
       ("pairs", segments)         ~800 boxes over the listed categories: rule taken
       ("total", n, segments)      exactly n valid boxes
       ("invalid", raw, bad, segs) raw entries of which `bad` are invalid (valid total = raw - bad)
       ("empty",) / ("single",)    0 boxes / 1 box
    Returns boxes [I][G][cap][4], valid [I][G][cap], counts [I][G]."""
    rng = np.random.default_rng(seed)
    out = []
    for kind in kinds:
        if kind[0] == "pairs":
            out.append(make_image(rng, G, cap, t, spread(800, kind[1], G)))
        elif kind[0] == "total":
            out.append(make_image(rng, G, cap, t, spread(kind[1], kind[2], G)))
        elif kind[0] == "invalid":
            raw, bad, segs = kind[1:]
            b, v, c = make_image(rng, G, cap, t, spread(raw, segs, G), touch_border=False)
            left = bad
            for g in segs:                       # exactly `bad` invalid entries at the segments' ends, none of them an edge pair's
                take = min(left, int(c[g]) - 64)
                v[g, int(c[g]) - take:int(c[g])] = 0
                left -= take
            assert left == 0
            out.append((b, v, c))
        elif kind[0] == "empty":
            out.append(make_image(rng, G, cap, t, np.zeros(G, np.int64)))
        elif kind[0] == "single":
            per = np.zeros(G, np.int64)
            per[G - 1] = 1
            out.append(make_image(rng, G, cap, t, per, edge_pairs=False, touch_border=False))
        else:
            raise ValueError(kind)
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]).astype(np.int32))
