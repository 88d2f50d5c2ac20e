"""Hand-built tables for the road cover vote (csrc/road_vote.h), shared by tests/test_road_votes_cpu.py and
tests/test_gpu_road_votes.py, and the numpy restatement both compare against.  A case is a dict of the tables
``raster_vote.TABLE_KEYS`` plus ``num_classes`` and ``threshold``; gt_cap is 128 throughout."""
import functools

import numpy as np

CAP = 128
THR32 = np.float32(0.3)                       # a score that IS the threshold, as the engine holds it
CLASS_COUNTS = (1, 2, 8)
# (I, A) of the first labels of the "edges" tables: m = rint(100 I / A) = 4, 5, 6 (the cut between 5 and 6 from both sides), the
# half-way 9/200, I = A, and A = 0 with I > 0; label 6 has I = 0
EDGE_PAIRS = ((5, 128), (7, 128), (8, 128), (9, 200), (50, 50), (3, 0), (0, 77))


def reference(b, K=None, threshold=None):
    """The rule of the issue, line by line: float64, detections in ascending order, np.round(I / A, 2)."""
    K = b["num_classes"] if K is None else K
    thr = b["threshold"] if threshold is None else threshold
    n, D = b["det_scores"].shape
    cap = b["gt_area"].shape[1]
    ws, wa, pairs = np.zeros((n, cap, K)), np.zeros((n, cap, K)), np.zeros((n, cap, K), np.int32)
    for t in range(n):
        G = min(int(b["tile_first"][t + 1] - b["tile_first"][t]), cap)
        for g in range(G):
            A = int(b["gt_area"][t, g])
            if A <= 0:
                continue
            for c in range(K):
                s_w, s_a, k = np.float64(0.0), np.float64(0.0), 0
                for d in range(min(max(int(b["det_count"][t]), 0), D)):
                    I = int(b["inter"][t, d, g])
                    if I <= 0 or int(b["det_classes"][t, d]) != c:
                        continue
                    frac = np.round(np.float64(I) / np.float64(A), 2)
                    score = np.float64(b["det_scores"][t, d])
                    if frac > 0.05 and score >= thr:
                        s_w = s_w + frac * score
                        s_a = s_a + frac
                        k += 1
                ws[t, g, c], wa[t, g, c], pairs[t, g, c] = s_w, s_a, k
    return ws, wa, pairs


def _random(rng, n, D, K, det_count, labels):
    b = {"det_scores": rng.uniform(0.05, 1.0, (n, D)).astype(np.float32),
         "det_classes": rng.integers(0, K + 1, (n, D)).astype(np.int32),         # K among them: votes for nothing
         "det_count": np.asarray(det_count, np.int32),
         "tile_first": np.concatenate([[0], np.cumsum(labels)]).astype(np.int32),
         "gt_area": rng.integers(1, 400, (n, CAP)).astype(np.int32),
         "num_classes": K}
    # about half of the pairs overlap, and the overlap is at most the label: I / A spreads over [0, 1]
    frac = rng.random((n, D, CAP)) * (rng.random((n, D, CAP)) < 0.5)
    b["inter"] = np.floor(frac * (b["gt_area"][:, None, :] + 1)).astype(np.int32).clip(0, b["gt_area"][:, None, :])
    return b


@functools.lru_cache(maxsize=None)
def case(name):
    """edges_k<K>_thr / edges_k<K>_zero: 3 tiles, 8 slots; tile 0 has 128 labels and all 8 slots in use, tile 1 no label, tile 2 one
    label.  slots_k<K>: tile 0 without detections, label counts 1, 40, 0.  slots100: 100 slots.  random4: 4 tiles, K = 2."""
    rng = np.random.default_rng(sum(map(ord, name)))        # a seed per case that does not depend on the process
    if name.startswith("edges_"):
        K = int(name.split("_")[1][1:])
        b = _random(rng, 3, 8, K, (8, 5, 3), (128, 0, 1))
        for g, (I, A) in enumerate(EDGE_PAIRS):
            b["gt_area"][0, g] = A
            b["inter"][0, :4, g] = I
        # slots 0..3 of tile 0 meet the edge labels: the score on the threshold in class 0, one ulp below it in class 0, class K - 1, class K
        b["det_scores"][0, 0] = THR32
        b["det_scores"][0, 1] = np.nextafter(THR32, np.float32(0))
        b["det_scores"][0, 2:4] = np.float32(0.75)
        b["det_classes"][0, :4] = (0, 0, K - 1, K)
        b["threshold"] = float(THR32) if name.endswith("_thr") else 0.0
        return b
    if name.startswith("slots_"):
        K = int(name.split("_")[1][1:])
        b = _random(rng, 3, 8, K, (0, 8, 2), (1, 40, 0))
        b["threshold"] = 0.3
        return b
    if name == "slots100":
        b = _random(rng, 2, 100, 2, (100, 37), (128, 63))
        b["threshold"] = 0.2
        return b
    if name == "random4":
        b = _random(rng, 4, 8, 2, (8, 1, 0, 6), (128, 17, 5, 64))
        b["threshold"] = 0.4
        return b
    raise KeyError(name)


CPU_NAMES = tuple(f"edges_k{K}_{w}" for K in CLASS_COUNTS for w in ("thr", "zero")) + tuple(f"slots_k{K}" for K in CLASS_COUNTS)
GPU_NAMES = CPU_NAMES + ("slots100", "random4")


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(case(name))


def same_bits(got, want):
    return all(np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w)
               for g, w in zip(got, want))
