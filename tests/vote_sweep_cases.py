"""Threshold lists and helpers for the vote sweep (csrc/road_vote.h, THE SWEEP), shared by tests/test_vote_sweep_cpu.py and
tests/test_gpu_vote_sweep.py.  The tables are those of tests/road_vote_cases.py."""
import numpy as np

from tests import road_vote_cases as V

REFERENCE = np.arange(0, 1., 0.05)                      # the reference's 20 thresholds
THR = float(V.THR32)
# a score that IS the threshold, the double just above it, 0, a duplicate of the first, and an unsorted pair (0.9 before 0.2)
MIXED = np.array([THR, np.nextafter(THR, 1.0), 0.0, THR, 0.9, 0.2], np.float64)
FULL = np.concatenate([MIXED, np.linspace(-0.25, 1.25, 26)])          # 32 entries: the capacity; below 0 and above 1 among them
ONE = np.array([THR], np.float64)
SLICE_NAMES = tuple(f"edges_k{K}_thr" for K in V.CLASS_COUNTS) + tuple(f"slots_k{K}" for K in V.CLASS_COUNTS)
LISTS = {"T1": ONE, "T20": REFERENCE, "T32": FULL}
assert FULL.size == 32 and MIXED[4] > MIXED[5]


def slice_of(tables, j):
    """Slice j of sweep tables (n, T, cap, K) -> (n, cap, K)."""
    return tuple(np.ascontiguousarray(a[:, j]) for a in tables)


def boundary_case():
    """One tile, one label of area 100, 20 detections of class 0 that each cover the label fully (frac 1): detection j scores the
    float32 rounding of REFERENCE[j].  With the sweep on REFERENCE, detection j votes in slice j exactly when
    float64(float32(t_j)) >= t_j."""
    n_det = REFERENCE.size
    b = {"det_scores": REFERENCE.astype(np.float32)[None].copy(), "det_classes": np.zeros((1, n_det), np.int32),
         "det_count": np.array([n_det], np.int32), "tile_first": np.array([0, 1], np.int32),
         "inter": np.zeros((1, n_det, V.CAP), np.int32), "gt_area": np.zeros((1, V.CAP), np.int32), "num_classes": 1}
    b["inter"][0, :, 0] = 100
    b["gt_area"][0, 0] = 100
    return b
