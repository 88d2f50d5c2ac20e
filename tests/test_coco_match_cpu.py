"""COCOeval's evaluateImg as the library states it (csrc/coco_match.h), the parts that need no GPU: the host restatement
``rs_host_coco_match`` against ``coco_eval.match_images`` on every case of tests/coco_match_cases.py, the C ABI's new entries and their
argument checks, the cases' own coverage of the rule, and the table layout's round trip.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from proj_roadsurf_amd import coco_eval, coco_match
from proj_roadsurf_amd.engine import load_library
from tests import coco_match_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_coco_match", "rs_host_coco_match", "rs_engine_fetch_eval_match_async", "rs_engine_fetch_eval_match_wait")
KINDS = ("bbox", "segm")
AREAS = tuple(coco_eval.AREA_RNG)


# ---------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name", M.NAMES)
def test_host_restatement_equals_match_images(name):
    b = M.case(name)
    t = coco_match.host_tables(b)
    n, D = b["det_scores"].shape
    for i in range(n):                                  # the order is a permutation of the slots in use, the rest is -1
        c = int(b["det_count"][i])
        assert sorted(t["order"][i, :c].tolist()) == list(range(c)) and (t["order"][i, c:] == -1).all()
        assert t["class_first"][i, 0] == 0 and t["class_first"][i, -1] == c
    pad = np.unpackbits(t["matched"].view(np.uint8) | t["ignored"].view(np.uint8), axis=-1, bitorder="little").reshape(n, 2, 4, 10, -1)
    for i in range(n):
        assert not pad[i, ..., int(b["det_count"][i]):].any()
    for kind in KINDS:
        assert M.records_equal(coco_match.records(b, t, kind), M.reference(name, kind))


# ---------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "rs_engine.h")).read()
    lib = load_library()
    for name in ENTRIES:
        assert f"int {name}(" in hdr, name
        assert hasattr(lib, name), name
    assert "typedef struct rs_eval_matches" in hdr
    assert lib.rs_abi_version() == 1


def test_entries_refuse_bad_arguments_before_touching_a_device():
    """No GPU here: a call that got past its argument checks would fail with a HIP error, or fault on the pointers, instead of these
    messages."""
    lib = load_library()
    err = lambda: lib.rs_last_error().decode()
    one = C.c_void_p(256)                               # never dereferenced: the checks come first
    thr = np.ascontiguousarray(coco_eval.IOU_THRS)
    good = [one] * 10 + [thr.ctypes.data, 1, 2, 100, 128] + [one] * 6
    for fn, tail in ((lib.rs_op_coco_match, [None]), (lib.rs_host_coco_match, [])):
        name = "rs_op_coco_match" if tail else "rs_host_coco_match"
        for i in list(range(11)) + list(range(15, 21)):
            bad = list(good)
            bad[i] = None
            assert fn(*bad, *tail) == -1 and "null" in err() and name in err(), (name, i, err())
        for i, values, code in ((11, (0, -1), -1), (12, (0, -3, 81), -1), (13, (0, -1), -1), (14, (0, -1), -1), (13, (1025,), -4), (14, (129,), -4)):
            for v in values:
                bad = list(good)
                bad[i] = v
                assert fn(*bad, *tail) == code and name in err(), (name, i, v, err())
    m = coco_match.empty_tables(1, 100, 2)
    assert lib.rs_engine_fetch_eval_match_async(None, 1, None, None, None, None, None, None, None, None, None, None) < 0
    assert "rs_engine_fetch_eval_match_async" in err()
    assert m["order"].shape == (1, 100) and m["matched"].shape == (1, 2, 4, 10, 4) and m["npig"].shape == (1, 2, 4, 2)


def test_parser_takes_the_third_mode_and_defaults_to_host():
    from proj_roadsurf_amd.train_model import build_parser
    ap = build_parser()
    assert ap.parse_args(["config.yaml"]).val_ap == "host"
    for mode in ("host", "device", "device-match"):
        assert ap.parse_args(["config.yaml", "--val-ap", mode]).val_ap == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["config.yaml", "--val-ap", "gpu"])


# ---------------------------------------------------------------------------------------------------- the cases themselves
def _rec(name, kind, key, tile=0):
    return M.reference(name, kind)[tile][key]


def _box_ious(b, t=0):
    c, g0, g1 = int(b["det_count"][t]), int(b["tile_first"][t]), int(b["tile_first"][t + 1])
    return coco_eval.box_iou(b["det_boxes"][t, :c].astype(np.float64), b["gt_boxes"][g0:g1], np.zeros(g1 - g0, bool))


def test_case_shapes_cover_the_boundaries():
    seen = {(int(b["det_count"][0]), int(b["tile_first"][1]), b["num_classes"]) for b in (M.case(n) for n in M.RANDOM)}
    assert {(d, g) for d, g, _ in seen} >= {(d, g) for d in M.DET_COUNTS for g in M.GT_COUNTS}
    assert {k for _, _, k in seen} == set(M.CATEGORIES) and all((100, 128, k) in seen for k in M.CATEGORIES)
    for name in M.RAGGED:
        b = M.case(name)
        assert len(b["det_count"]) == 3 and b["det_count"][1] == 0 and b["tile_first"][2] == b["tile_first"][1]


def test_random_families_are_not_empty():
    """At least a quarter of the random families' detections are matched at IoU 0.5 and some are unmatched at 0.95, per kind; every
    random tile that has both a detection and a ground truth matches at least one at 0.5."""
    for kind in KINDS:
        for family in (M.RANDOM, M.RAGGED):
            dets = hit50 = miss95 = 0
            for name in family:
                b = M.case(name)
                for t, rec in enumerate(M.reference(name, kind)):
                    here = sum(int(rec[(c, "all")][1][0].sum()) for c in range(b["num_classes"]) if (c, "all") in rec)
                    hit50 += here
                    miss95 += sum(int((~rec[(c, "all")][1][9]).sum()) for c in range(b["num_classes"]) if (c, "all") in rec)
                    dets += int(b["det_count"][t])
                    if b["det_count"][t] and b["tile_first"][t + 1] > b["tile_first"][t] and b["num_classes"] <= 2:
                        assert here >= 1, (name, t, kind)
            print(f"{kind}: {dets} detections, {hit50} matched at 0.5, {miss95} unmatched at 0.95")
            assert 4 * hit50 >= dets and miss95 >= 1, (kind, dets, hit50, miss95)


def test_random_families_exercise_the_walk():
    """Somewhere in the random families: a detection matched to an ignored ground truth, an unmatched detection ignored for its own
    area, an unmatched detection that is a plain false positive, and tied scores inside a category."""
    to_ignored = ignored_unmatched = false_pos = tied = 0
    for name in list(M.RANDOM) + list(M.RAGGED):
        b = M.case(name)
        for t, rec in enumerate(M.reference(name, "bbox")):
            for (c, a), (s, m, ig, _) in rec.items():
                to_ignored += int((m & ig).sum())
                ignored_unmatched += int((~m & ig).sum())
                false_pos += int((~m & ~ig).sum())
                tied += int(a == "all" and len(np.unique(s)) < len(s))
    assert to_ignored and ignored_unmatched and false_pos and tied, (to_ignored, ignored_unmatched, false_pos, tied)


def test_constructed_tied_scores():
    b = M.case("tied_scores")
    s0, m0, _, _ = _rec("tied_scores", "bbox", (0, "all"))
    assert np.array_equal(s0, [0.5, 0.5, 0.5]) and np.array_equal(_rec("tied_scores", "bbox", (1, "all"))[0], [np.float64(np.float32(0.9)), 0.5, 0.5])
    # slot order inside the tie: slot 1 (IoU 1) stands before slot 2 (IoU 0.952) and takes their ground truth at every threshold
    assert m0[:, 0].all() and m0[:, 1].all() and not m0[:, 2].any()
    assert _box_ious(b)[2, 0] >= 0.95
    t = coco_match.host_tables(b)
    assert t["order"][0, :6].tolist() == [0, 1, 2, 5, 3, 4] and t["class_first"][0].tolist() == [0, 3, 6]


def test_constructed_tied_iou_takes_the_later_ground_truth():
    iou = _box_ious(M.case("tied_iou"))
    assert iou[0, 0] == iou[0, 1] == 0.6 and iou[1, 0] == 0.7 and iou[1, 1] < 0.5
    for kind in KINDS:
        m = _rec("tied_iou", kind, (0, "all"))[1]
        assert m[:3, 0].all() and not m[3:, 0].any()              # 0.5, 0.55, 0.6
        assert m[:5, 1].all() and not m[5:, 1].any()              # detection 1 finds ground truth 0 free: the later one was taken


def test_constructed_ious_on_thresholds():
    iou = _box_ious(M.case("iou_on_thresholds"))
    assert iou[0, 0] == coco_eval.IOU_THRS[0] and iou[1, 1] == coco_eval.IOU_THRS[5] and iou[2, 2] == coco_eval.IOU_THRS[6]
    for kind in KINDS:
        assert [int(_rec("iou_on_thresholds", kind, (c, "all"))[1].sum()) for c in range(3)] == [1, 6, 7]


def test_constructed_area_edges():
    for kind in KINDS:
        assert [_rec("area_edges", kind, (0, a))[3] for a in AREAS] == [2, 1, 2, 1]      # 1024: small and medium; 9216: medium and large
        ig = {a: _rec("area_edges", kind, (0, a))[2] for a in AREAS}
        assert not ig["all"].any() and not ig["medium"].any() and ig["small"][:, 1].all() and ig["large"][:, 0].all()


def test_constructed_best_ground_truth_is_ignored():
    iou = _box_ious(M.case("best_is_ignored"))
    assert iou[0, 0] == 1.0 and iou[0, 1] == 0.5625
    for kind in KINDS:
        _, m, ig, n = _rec("best_is_ignored", kind, (0, "small"))
        assert n == 1 and m[:, 0].all()
        assert not ig[:2, 0].any() and ig[2:, 0].all()       # the kept, worse one up to 0.55 (early stop); then the ignored one
        _, m1, ig1, n1 = _rec("best_is_ignored", kind, (1, "small"))
        assert n1 == 0 and m1.all() and ig1.all()            # matched to an ignored ground truth


def test_constructed_outside_range_unmatched():
    for kind in KINDS:
        flags = {a: _rec("outside_range_unmatched", kind, (0, a)) for a in AREAS}
        assert not any(f[1].any() for f in flags.values())
        assert flags["small"][2].all() and flags["medium"][2].all() and not flags["all"][2].any() and not flags["large"][2].any()


def test_constructed_competing_detections():
    iou = _box_ious(M.case("competing"))
    assert iou[0, 0] >= 0.9 and iou[1, 0] == 1.0
    for kind in KINDS:
        s, m, ig, n = _rec("competing", kind, (0, "all"))
        assert s[0] > s[1] and m[:, 0].all() and not m[:, 1].any() and n == 1      # the ground truth is skipped once matched


def test_constructed_other_category():
    for kind in KINDS:
        rec = M.reference("other_category", kind)[0]
        assert set(rec) == {(c, a) for c in (0, 1) for a in AREAS}
        assert rec[(0, "all")][1].shape == (10, 3) and not rec[(0, "all")][1].any() and rec[(0, "all")][3] == 0
        assert rec[(1, "all")][1].shape == (10, 0) and rec[(1, "all")][3] == 3


# ---------------------------------------------------------------------------------------------------- layout round trip
def pack_records(recs, scores, classes, count, K, D):
    """numpy packer of one tile's ``match_images`` records (bbox, segm) into the table layout of csrc/coco_match.h."""
    t = {k: v[0] for k, v in coco_match.empty_tables(1, D, K).items()}
    cls = np.where((classes[:count] >= 0) & (classes[:count] < K), classes[:count], K)
    order = np.lexsort((np.arange(count), -scores[:count].astype(np.float64), cls))
    t["order"][:] = -1
    t["order"][:count] = order
    t["class_first"][:] = [int((cls < c).sum()) for c in range(K + 1)]
    for kind, rec in enumerate(recs):
        for (c, a), (s, m, ig, n) in rec.items():
            ai, p0 = AREAS.index(a), int(t["class_first"][c])
            assert np.array_equal(s, scores[order[p0:p0 + len(s)]].astype(np.float64))
            for name, flags in (("matched", m), ("ignored", ig)):
                for ti, p in zip(*np.nonzero(flags)):
                    t[name][kind, ai, ti, (p0 + p) >> 5] |= np.uint32(1) << np.uint32((p0 + p) & 31)
            t["npig"][kind, ai, c] = n
    return t


@pytest.mark.parametrize("name", ["random_d100_g128_k2", "random_d65_g63_k8", "random_d100_g128_k80", "ragged_small_tables", "tied_scores"])
def test_records_round_trip_through_the_layout(name):
    b = M.case(name)
    K, D = b["num_classes"], b["det_scores"].shape[1]
    host = coco_match.host_tables(b)
    for i in range(len(b["det_count"])):
        want = [M.reference(name, kind)[i] for kind in KINDS]
        t = pack_records(want, b["det_scores"][i], b["det_classes"][i], int(b["det_count"][i]), K, D)
        t["gt_per_class"][:] = np.bincount(b["gt_classes"][b["tile_first"][i]:b["tile_first"][i + 1]], minlength=K)
        for k in ("order", "class_first", "matched", "ignored", "npig", "gt_per_class"):      # the packer writes what the library writes
            assert np.array_equal(t[k], host[k][i]), (k, i)
        for kind, w in zip(KINDS, want):
            got = coco_eval.records_from_tables(b["det_scores"][i], *[t[k] for k in coco_match.TABLES], iou_type=kind)
            assert M.records_equal([got], [w])
