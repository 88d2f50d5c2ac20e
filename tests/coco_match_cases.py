"""Detection / ground-truth batches for the device matcher's tests (tests/test_coco_match_cpu.py, tests/test_gpu_coco_match.py): each
case is a batch dict as proj_roadsurf_amd/coco_match.py describes it.  Masks are axis-aligned integer rectangles, so the three count
tables are exact rectangle arithmetic; the boxes are those rectangles with a sub-pixel jitter (float32 for detections, float64 for ground
truths) unless a constructed case needs exact values.  Slots at or past a tile's count hold plausible garbage: nothing may read them.

RANDOM: every pair of (detections, ground truths) per tile out of 0, 1, 63, 64, 65, 100 x 0, 1, 63, 64, 65, 128, the category count
cycling through 1, 2, 8, 80 (each of them also at the full 100 x 128), one tile per call; RAGGED: three tiles per call with an empty
tile in the middle; CAPACITY: more slots than the order pass has lanes, and the kernels' 1024 slots; CONSTRUCTED: one family per rule of
csrc/coco_match.h."""
import functools

import numpy as np

D_SLOTS, GT_CAP, SIDE = 100, 128, 256
DET_COUNTS = (0, 1, 63, 64, 65, 100)
GT_COUNTS = (0, 1, 63, 64, 65, 128)
CATEGORIES = (1, 2, 8, 80)


def _rect_inter(a, b):
    """(d, 4) x (g, 4) integer XYXY rectangles -> (d, g) pixel counts of the intersections."""
    w = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    h = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    return (w * h).astype(np.int32)


def _area(r):
    return ((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1])).astype(np.int32)


def tile(db=(), ds=(), dc=(), gb=(), gc=(), dm=None, gm=None):
    """One tile: detection boxes / scores / classes, ground-truth boxes / classes, and the integer rectangles that stand for the masks
    (default: the boxes rounded)."""
    db, gb = np.asarray(db, np.float32).reshape(-1, 4), np.asarray(gb, np.float64).reshape(-1, 4)
    dm = np.rint(db).astype(np.int64) if dm is None else np.asarray(dm, np.int64).reshape(-1, 4)
    gm = np.rint(gb).astype(np.int64) if gm is None else np.asarray(gm, np.int64).reshape(-1, 4)
    return dict(db=db, ds=np.asarray(ds, np.float32), dc=np.asarray(dc, np.int32), gb=gb, gc=np.asarray(gc, np.int32), dm=dm, gm=gm)


def batch(tiles, K, D=D_SLOTS, cap=GT_CAP, seed=0):
    rng = np.random.default_rng([seed, len(tiles), K])
    n = len(tiles)
    b = {"num_classes": K,
         "det_boxes": rng.uniform(0, SIDE, (n, D, 4)).astype(np.float32), "det_scores": rng.random((n, D)).astype(np.float32),
         "det_classes": rng.integers(0, K, (n, D)).astype(np.int32), "det_count": np.array([len(t["ds"]) for t in tiles], np.int32),
         "gt_boxes": np.concatenate([t["gb"] for t in tiles]), "gt_classes": np.concatenate([t["gc"] for t in tiles]).astype(np.int32),
         "tile_first": np.concatenate([[0], np.cumsum([len(t["gc"]) for t in tiles])]).astype(np.int32),
         "inter": np.zeros((n, D, cap), np.int32), "det_area": np.zeros((n, D), np.int32), "gt_area": np.zeros((n, cap), np.int32)}
    for i, t in enumerate(tiles):
        d, g = len(t["ds"]), len(t["gc"])
        assert d <= D and g <= cap
        b["det_boxes"][i, :d], b["det_scores"][i, :d], b["det_classes"][i, :d] = t["db"], t["ds"], t["dc"]
        b["inter"][i, :d, :g] = _rect_inter(t["dm"], t["gm"])
        b["det_area"][i, :d], b["gt_area"][i, :g] = _area(t["dm"]), _area(t["gm"])
    return b


def _rects(rng, k):
    lo = rng.integers(0, SIDE - 8, (k, 2))
    size = np.where(rng.random((k, 2)) < 0.5, rng.integers(6, 40, (k, 2)), rng.integers(30, 150, (k, 2)))
    return np.concatenate([lo, np.minimum(lo + size, SIDE)], 1).astype(np.int64)


def random_tile(rng, d, g, K):
    """g ground truths over all three area ranges; about 0.8 min(d, g) detections sit on a ground truth of their own, moved by up to two
    pixels (a third of them not at all: IoU exactly 1), mostly in its category; the rest are anywhere.  Scores have two decimals."""
    gm, gc = _rects(rng, g), rng.integers(0, K, g)
    dm, dc = _rects(rng, d), rng.integers(0, K, d)
    hits = min(g, d, int(0.8 * min(d, g)) + 1)
    for i, j in zip(rng.permutation(d)[:hits], rng.permutation(g)[:hits]):
        r = gm[j] + (0 if rng.random() < 0.33 else rng.integers(-2, 3, 4))
        r[2:] = np.maximum(r[2:], r[:2] + 1)
        dm[i] = np.clip(r, 0, SIDE)
        if dm[i][2] <= dm[i][0] or dm[i][3] <= dm[i][1]:
            dm[i] = gm[j]
        if rng.random() < 0.9:
            dc[i] = gc[j]
    db = (dm + rng.uniform(-0.4, 0.4, (d, 4))).astype(np.float32)
    gb = gm + rng.uniform(-0.4, 0.4, (g, 4))
    return tile(db, np.round(rng.random(d), 2), dc, gb, gc, dm, gm)


def _random_case(d, g, K, seed):
    return lambda: batch([random_tile(np.random.default_rng([seed, d, g, K]), d, g, K)], K, seed=seed)


def _ragged_case(shapes, K, seed, D=D_SLOTS, cap=GT_CAP):
    return lambda: batch([random_tile(np.random.default_rng([seed, i, d, g, K]), d, g, K) for i, (d, g) in enumerate(shapes)], K, D, cap, seed)


RANDOM = {}
for _i, _d in enumerate(DET_COUNTS):
    for _j, _g in enumerate(GT_COUNTS):
        _K = CATEGORIES[(_i + _j) % 4]
        RANDOM[f"random_d{_d}_g{_g}_k{_K}"] = _random_case(_d, _g, _K, 11)
for _K in CATEGORIES:
    RANDOM.setdefault(f"random_d100_g128_k{_K}", _random_case(100, 128, _K, 12))

RAGGED = {
    "ragged_65_0_100": _ragged_case([(65, 64), (0, 0), (100, 128)], 2, 21),
    "ragged_dets_without_gts": _ragged_case([(64, 0), (0, 0), (0, 65)], 8, 22),
    "ragged_k80": _ragged_case([(100, 63), (0, 0), (63, 128)], 80, 23),
    "ragged_small_tables": _ragged_case([(33, 70), (0, 0), (40, 5)], 3, 24, D=40, cap=70),      # slots and gt_cap below the capacities, W = 2
}

# more slots than the order pass has lanes (256), and the kernels' capacity (1024 slots, 32 flag words per row)
CAPACITY = {
    "slots_300": _ragged_case([(257, 65)], 2, 31, D=300),
    "slots_1024": _ragged_case([(1024, 40), (0, 0), (700, 128)], 8, 32, D=1024),
}

SQ = [0.0, 0.0, 40.0, 40.0]


def _tied_scores():
    # three detections of category 0 and two of category 1 share the score 0.5; slot order decides inside a category
    gb = [[10, 10, 50, 50], [60, 60, 100, 100], [10, 60, 50, 100]]
    db = [[60, 60, 100, 100], [10, 10, 50, 50], [10, 10, 50, 52], [10, 60, 50, 100], [10, 60, 50, 98], [200, 200, 220, 220]]
    return batch([tile(db, [0.5, 0.5, 0.5, 0.5, 0.5, 0.9], [0, 0, 0, 1, 1, 1], gb, [0, 0, 1])], 2, D=8)


def _tied_iou():
    # detection 0 overlaps ground truths 0 and 1 with the same IoU (0.6): it takes the LATER one.  Detection 1 (lower score) reaches only
    # ground truth 0 and finds it free.  Were the earlier one taken, detection 1 would stay unmatched.
    gb = [[0, 0, 40, 40], [20, 0, 60, 40]]
    db = [[10, 0, 50, 40], [0, 0, 40, 28]]
    return batch([tile(db, [0.9, 0.8], [0, 0], gb, [0, 0])], 1, D=8)


def _iou_on_thresholds():
    # IoU 0.5, 0.75 and 0.8 exactly, one category each: matched at 1, 6 and 7 of the 10 thresholds
    return batch([tile([[0, 0, 40, 20], [0, 0, 40, 30], [0, 0, 40, 32]], [0.9, 0.9, 0.9], [0, 1, 2], [SQ, SQ, SQ], [0, 1, 2])], 3, D=8)


def _area_edges():
    # ground-truth areas exactly 32^2 (small and medium) and 96^2 (medium and large), each with a detection on it
    gb = [[0, 0, 32, 32], [100, 100, 196, 196]]
    return batch([tile(gb, [0.9, 0.8], [0, 0], gb, [0, 0])], 1, D=8)


def _best_is_ignored():
    # detection 0: IoU 1 with a 40 x 40 ground truth (ignored in "small"), IoU 0.5625 with a 30 x 30 one inside it.  In "small", up to
    # threshold 0.55, the worse but kept one is taken and the walk stops in front of the ignored ones; from 0.6 on only the ignored one
    # passes, and the detection is matched to it and ignored.  Detection 1 (category 1) sits on a 120 x 120 ground truth alone: in
    # "small" and "medium" it is matched to an ignored ground truth and ignored.
    gb = [[0, 0, 40, 40], [0, 0, 30, 30], [100, 100, 220, 220]]
    db = [[0, 0, 40, 40], [100, 100, 220, 220]]
    return batch([tile(db, [0.9, 0.8], [0, 1], gb, [0, 0, 1])], 2, D=8)


def _outside_range_unmatched():
    # a large detection with nothing under it: unmatched, ignored in "small" and "medium", a false positive in "all" and "large"
    return batch([tile([[50, 50, 200, 200]], [0.7], [0], [[0, 0, 20, 20]], [0])], 1, D=8)


def _competing():
    # two detections on one ground truth: the higher score takes it, the other one passes every threshold up to 0.9 and is unmatched
    return batch([tile([[0, 0, 40, 38], [0, 0, 40, 40]], [0.6, 0.9], [0, 0], [SQ], [0])], 1, D=8)


def _other_category():
    # every detection in category 0, every ground truth in category 1 (same places)
    gb = [[0, 0, 40, 40], [50, 50, 90, 90], [100, 0, 140, 40]]
    return batch([tile(gb, [0.9, 0.8, 0.7], [0, 0, 0], gb, [1, 1, 1])], 2, D=8)


CONSTRUCTED = {"tied_scores": _tied_scores, "tied_iou": _tied_iou, "iou_on_thresholds": _iou_on_thresholds, "area_edges": _area_edges,
               "best_is_ignored": _best_is_ignored, "outside_range_unmatched": _outside_range_unmatched, "competing": _competing,
               "other_category": _other_category}

CASES = {**RANDOM, **RAGGED, **CAPACITY, **CONSTRUCTED}
NAMES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name, iou_type):
    """coco_eval.match_images on the case, computed once and shared; nobody changes it."""
    from proj_roadsurf_amd import coco_eval
    from proj_roadsurf_amd.coco_match import images
    b = case(name)
    gts, dts = images(b)
    return coco_eval.match_images(gts, dts, b["num_classes"], iou_type, b["det_scores"].shape[1])


def records_equal(got, want):
    """Exact: the key sets, the scores, both flag arrays and the count."""
    assert len(got) == len(want)
    for t, (ra, rb) in enumerate(zip(got, want)):
        assert ra.keys() == rb.keys(), (t, sorted(set(ra) ^ set(rb)))
        for k in ra:
            for i, (x, y) in enumerate(zip(ra[k], rb[k])):
                x, y = np.asarray(x), np.asarray(y)
                assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), (t, k, i)
    return True
