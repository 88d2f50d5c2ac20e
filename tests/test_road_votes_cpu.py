"""The road cover vote as the library states it (csrc/road_vote.h), the parts that need no GPU: the host restatement
``rs_host_road_votes`` against a numpy restatement on hand-built tables (tests/road_vote_cases.py), every double compared by its bits;
``reduce_votes`` against the reference's own two steps (``weighted_scores``, ``determine_detected_class``); the C ABI's new entries,
their structures and their argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd.engine import RsRoadVotes, load_library
from tests import road_vote_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_road_votes", "rs_host_road_votes", "rs_engine_fetch_votes_async", "rs_engine_fetch_votes_wait")


# ---------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", V.CPU_NAMES)
def test_host_restatement_equals_numpy_bit_for_bit(name):
    b = V.case(name)
    want = V.expected(name)
    got = RV.road_votes_host(b, b["num_classes"], b["threshold"], prefill=0.0)
    again = RV.road_votes_host(b, b["num_classes"], b["threshold"], prefill=7.0)      # whatever the buffers held: every cell is written
    assert V.same_bits(got, want), [int((g != w).sum()) for g, w in zip(got, want)]
    assert V.same_bits(again, want)
    n = len(b["det_count"])
    for t in range(n):                                                                 # rows past the tile's own labels are zero
        G = int(b["tile_first"][t + 1] - b["tile_first"][t])
        assert not got[0][t, G:].any() and not got[1][t, G:].any() and not got[2][t, G:].any()
    assert want[2].sum() > 0


def test_numpy_route_equals_the_restatement():
    """``votes_from_counts`` (the vectorised rule ``vote_tables_host`` ends with) gives the same bits as the cell-by-cell loop."""
    for name in ("edges_k2_thr", "edges_k8_zero", "slots_k2"):
        b, want = V.case(name), V.expected(name)
        for t in range(len(b["det_count"])):
            G, c = int(b["tile_first"][t + 1] - b["tile_first"][t]), int(b["det_count"][t])
            got = RV.votes_from_counts(b["inter"][t, :c, :G], b["gt_area"][t, :G], b["det_scores"][t, :c], b["det_classes"][t, :c],
                                       b["num_classes"], b["threshold"])
            assert V.same_bits(got, [w[t, :G] for w in want]), (name, t)


def test_edge_cells_are_what_the_rule_says():
    """The hand-built slots 0..3 of the ``edges`` tables alone (det_count cut to 4), read off the restatement AND the library: which
    side of every cut a pair falls on.  Slot 0 scores exactly the threshold (class 0), slot 1 one ulp less (class 0), slot 2 is of
    class K - 1, slot 3 of class K."""
    assert [int(np.rint(np.float64(I) / np.float64(A) * 100.0)) for I, A in V.EDGE_PAIRS[:5]] == [4, 5, 6, 4, 100]
    for K in V.CLASS_COUNTS:
        for which, in_class0 in (("thr", 1 + (K == 1)), ("zero", 2 + (K == 1))):
            b = dict(V.case(f"edges_k{K}_{which}"))
            b["det_count"] = np.array([4, 0, 0], np.int32)
            want = V.reference(b)
            assert V.same_bits(RV.road_votes_host(b, K, b["threshold"]), want)
            ws, wa, pairs = want
            assert pairs[0, :7, 0].tolist() == [0, 0, in_class0, 0, in_class0, 0, 0], (K, which)
            if K > 1:
                assert pairs[0, :7, K - 1].tolist() == [0, 0, 1, 0, 1, 0, 0] and pairs[0, :7, 1:K - 1].sum() == 0
                assert wa[0, 4, K - 1] == 1.0 and ws[0, 4, K - 1] == np.float64(np.float32(0.75))      # I == A: frac 1
                if which == "thr":
                    assert wa[0, 4, 0] == 1.0 and ws[0, 4, 0] == np.float64(V.THR32)
            assert pairs.sum() == pairs[0].sum()


# ---------------------------------------------------------------------------------------------------- from tables to roads
def _scene():
    """Two tiles.  Tile 0: roads a, tie, none, split, thr; tile 1: split (its second piece), b.  inter as (labels, detections)."""
    t0 = dict(ids=["a", "tie", "none", "split", "thr"], area=np.array([100, 100, 100, 200, 100]),
              scores=np.array([0.9, 0.6, 0.6, 0.35], np.float32), classes=np.array([0, 1, 0, 1]),
              inter=np.array([[60, 30, 0, 20],          # a: artificial 0.6 * 0.9, natural 0.3 * 0.6 and 0.2 * 0.35
                              [0, 50, 50, 0],           # tie: one pair per class, same weight, same score
                              [0, 0, 0, 0],             # none: nothing overlaps
                              [80, 0, 0, 30],           # split: first piece
                              [70, 0, 0, 40]]))         # thr: its only natural pair scores 0.35
    t1 = dict(ids=["split", "b"], area=np.array([300, 64]),
              scores=np.array([0.8, 0.7, 0.45], np.float32), classes=np.array([1, 0, 1]),
              inter=np.array([[120, 31, 0],             # split: second piece
                              [0, 7, 64]]))
    return [t0, t1]


def _both(threshold, class_names=RV.CLASS_NAMES):
    tiles = _scene()
    rows = [r for t in tiles for r in RV.weighted_scores(t["inter"], t["area"], t["scores"], t["classes"], t["ids"])]
    want = RV.determine_detected_class(rows, [rid for t in tiles for rid in t["ids"]], threshold)
    tables = [RV.votes_from_counts(t["inter"].T, t["area"], t["scores"], t["classes"], len(class_names), threshold) for t in tiles]
    return want, RV.reduce_votes(tables, [t["ids"] for t in tiles], class_names)


@pytest.mark.parametrize("threshold", [0.0, 0.5])
def test_reduce_votes_equals_the_reference_steps(threshold):
    """Roads that lie in one tile compare with ==.  (Their sums are the same sequential float64 sums on both sides: Python's ``sum``
    over the road's rows in detection order, and at most two pairs per class here, so a compensated ``sum`` would round alike.)"""
    want, got = _both(threshold)
    assert [w["road_id"] for w in want] == [g["road_id"] for g in got] == ["a", "tie", "none", "split", "thr", "b"]
    for w, g in zip(want, got):
        if w["road_id"] != "split":
            assert w == g, (w, g)
            continue
        assert w["cover_type"] == g["cover_type"] and set(w) == set(g)
        for k in ("nat_score", "art_score", "diff_score"):
            assert abs(w[k] - g[k]) <= 1e-12, (k, w, g)
    by = {g["road_id"]: g for g in got}
    assert by["tie"]["cover_type"] == "undetermined" and by["tie"]["diff_score"] == 0
    assert by["none"] == {"road_id": "none", "cover_type": "undetected", "nat_score": 0, "art_score": 0, "diff_score": 0}
    assert by["split"]["cover_type"] in ("artificial", "natural")
    if threshold == 0.5:            # the natural pairs of `thr` (0.35) and of `a` (0.35 only) fall out; `thr` keeps one class
        assert by["thr"]["nat_score"] == 0 and by["thr"]["cover_type"] == "artificial" and by["thr"]["art_score"] == 0.9
    else:
        assert by["thr"]["nat_score"] == round(float(np.float32(0.35)), 3)


def test_reduce_votes_from_the_library_tables():
    """The same road table from ``rs_host_road_votes``' padded tables."""
    tiles = _scene()
    D = 4
    b = {"det_scores": np.zeros((2, D), np.float32), "det_classes": np.zeros((2, D), np.int32), "det_count": np.array([4, 3], np.int32),
         "tile_first": np.array([0, 5, 7], np.int32), "inter": np.zeros((2, D, 128), np.int32), "gt_area": np.zeros((2, 128), np.int32)}
    for i, t in enumerate(tiles):
        c, g = len(t["scores"]), len(t["ids"])
        b["det_scores"][i, :c], b["det_classes"][i, :c] = t["scores"], t["classes"]
        b["inter"][i, :c, :g], b["gt_area"][i, :g] = t["inter"].T, t["area"]
    ws, wa, pairs = RV.road_votes_host(b, 2, 0.5)
    got = RV.reduce_votes([(ws[i, :len(t["ids"])], wa[i, :len(t["ids"])], pairs[i, :len(t["ids"])]) for i, t in enumerate(tiles)], [t["ids"] for t in tiles])
    assert got == _both(0.5)[1]


def test_reduce_votes_with_another_class_list():
    names = {0: "asphalt", 1: "gravel", 2: "grass"}
    ws = np.array([[0.5, 0.2, 0.0], [0.3, 0.3, 0.0], [0.0, 0.0, 0.0]])
    wa = np.array([[1.0, 0.25, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0]])
    pairs = np.array([[2, 1, 0], [1, 1, 0], [0, 0, 0]], np.int32)
    got = RV.reduce_votes([(ws, wa, pairs)], [["r1", "r2", "r3"]], names)
    assert got[0] == {"road_id": "r1", "cover_type": "gravel", "asphalt_score": 0.5, "gravel_score": 0.8, "grass_score": 0, "diff_score": 0.8 - 0.5}
    assert got[1]["cover_type"] == "undetermined" and got[1]["diff_score"] == 0 and got[1]["asphalt_score"] == got[1]["gravel_score"] == 0.6
    assert got[2] == {"road_id": "r3", "cover_type": "undetected", "asphalt_score": 0, "gravel_score": 0, "grass_score": 0, "diff_score": 0}


def test_reduce_votes_is_linear_in_roads():
    """20 000 roads, each with a piece in two tiles: a per-road scan of the pieces (the ``rid in seen`` of the restatement) would take
    minutes here; the reduction takes a fraction of a second.  Every road's index is 0.5 by construction."""
    R = 20000
    rng = np.random.default_rng(1)
    wa = rng.random((R, 2)) + 0.1
    half = (wa * 0.5, wa, np.ones((R, 2), np.int32))
    got = RV.reduce_votes([half, half], [list(range(R)), list(range(R))[::-1]])
    assert len(got) == R and [g["road_id"] for g in got[:3]] == [0, 1, 2]
    assert all(g["cover_type"] != "undetected" and g["nat_score"] == g["art_score"] == 0.5 for g in got)


# ---------------------------------------------------------------------------------------------------- ABI
def test_header_library_and_ctypes_agree():
    hdr = open(os.path.join(ROOT, "include", "rs_engine.h")).read()
    lib = load_library()
    for name in ENTRIES:
        assert f"int {name}(" in hdr, name
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct rs_road_votes \{(.*?)\} rs_road_votes;", hdr, re.S).group(1)
    fields = re.findall(r"(double|int32_t)\*\s+(\w+);", body)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, C.POINTER(ctype[t])) for t, n in fields] == list(RsRoadVotes._fields_)
    assert C.sizeof(RsRoadVotes) == 4 * C.sizeof(C.c_void_p)
    for name, count in (("rs_op_road_votes", 15), ("rs_host_road_votes", 14), ("rs_engine_fetch_votes_async", 9), ("rs_engine_fetch_votes_wait", 1)):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == count == len(getattr(lib, name).argtypes), name
    src = open(os.path.join(ROOT, "proj_roadsurf_amd", "csrc", "road_vote.h")).read()
    assert "#define RV_MAX_GT 128" in src and "#define RS_EVAL_GT_CAP 128" in hdr
    assert lib.rs_abi_version() == 1


def test_entries_refuse_bad_arguments_before_touching_anything():
    """No GPU here and the pointers are not memory: a call that got past its checks would fault or fail with a HIP error."""
    lib = load_library()
    err = lambda: lib.rs_last_error().decode()
    one = C.c_void_p(256)
    good = [one] * 6 + [1, 2, 100, 128, 0.0] + [one] * 3
    for fn, tail in ((lib.rs_op_road_votes, [None]), (lib.rs_host_road_votes, [])):
        name = "rs_op_road_votes" if tail else "rs_host_road_votes"
        for i in list(range(6)) + [11, 12, 13]:
            bad = list(good)
            bad[i] = None
            assert fn(*bad, *tail) == -1 and "null" in err() and name in err(), (name, i, err())
        for i, values, code in ((6, (0, -1), -1), (7, (0, -3, 81), -1), (8, (0, -1), -1), (9, (0, -1), -1),
                                (10, (float("nan"), float("inf"), -float("inf")), -1), (8, (1025,), -4), (9, (129,), -4)):
            for v in values:
                bad = list(good)
                bad[i] = v
                assert fn(*bad, *tail) == code and name in err(), (name, i, v, err())
    assert lib.rs_engine_fetch_votes_async(None, 1, None, None, None, None, None, 0.0, None) < 0 and "rs_engine_fetch_votes_async" in err()
    assert lib.rs_engine_fetch_votes_wait(None) < 0
