"""``proj_roadsurf_amd/road_metrics.py`` (the reference's final_metrics.py on road tables): every rule against a brute-force statement
written here, the choosers on hand-written sequences, and the whole route on the CPU -- sweep tables of a hand-built scene against
the reference's row route (``weighted_scores``, ``determine_detected_class``) per threshold."""
import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd import road_metrics as M

CLASSES = ["artificial", "natural"]


def test_tag_on_all_five_combinations():
    assert M.tag("undetermined", "artificial") == "FN" and M.tag("undetected", "natural") == "FN"
    assert M.tag("artificial", "artificial") == "TP" and M.tag("natural", "natural") == "TP"
    assert M.tag("natural", "artificial") == "wrong class"


def _brute(rows, categories, classes):
    """The issue's counts, one comprehension per number."""
    rows = [r for r in rows if categories.get(r["road_id"]) in classes]
    tagged = [(M.tag(r["cover_type"], categories[r["road_id"]]), r["cover_type"], categories[r["road_id"]]) for r in rows]
    out = []
    for k in classes:
        tp = sum(1 for t, c, g in tagged if t == "TP" and g == k)
        fp = sum(1 for t, c, g in tagged if t == "wrong class" and c == k)
        fn = sum(1 for t, c, g in tagged if t == "FN" and g == k) + sum(1 for t, c, g in tagged if t == "wrong class" and g == k)
        pk, rk = (tp / (tp + fp), tp / (tp + fn)) if tp else (0, 0)
        out.append({"cover_class": k, "TP": tp, "FP": fp, "FN": fn, "Pk": pk, "Rk": rk, "f1k": 2 * pk * rk / (pk + rk) if tp else 0,
                    "count": sum(1 for t, c, g in tagged if g == k)})
    total = sum(o["count"] for o in out)
    pw = sum(o["Pk"] * o["count"] for o in out) / total
    rw = sum(o["Rk"] * o["count"] for o in out) / total
    pb, rb = sum(o["Pk"] for o in out) / len(classes), sum(o["Rk"] for o in out) / len(classes)
    f1 = lambda p, r: 0 if p == 0 and r == 0 else 2 * p * r / (p + r)
    return out, {"Pw": pw, "Rw": rw, "f1w": f1(pw, rw), "Pb": pb, "Rb": rb, "f1b": f1(pb, rb)}


def _random_rows(seed, n=60, classes=CLASSES, extra=("undetermined", "undetected")):
    rng = np.random.default_rng(seed)
    covers = list(classes) + list(extra)
    rows = [{"road_id": i, "cover_type": covers[int(rng.integers(len(covers)))], "diff_score": float(rng.random())} for i in range(n)]
    cats = {i: (list(classes) + ["track"])[int(rng.integers(len(classes) + 1))] for i in range(n)}      # "track": not among the classes
    return rows, cats


@pytest.mark.parametrize("classes", [CLASSES, ["asphalt", "gravel", "grass"]])
def test_metrics_equal_a_brute_force_count(classes):
    for seed in range(4):
        rows, cats = _random_rows(seed, classes=classes)
        assert M.metrics(rows, cats, classes) == _brute(rows, cats, classes)
    by_class, glob = M.metrics(rows, cats, classes)
    assert sum(c["count"] for c in by_class) == sum(1 for v in cats.values() if v in classes) < len(rows)    # "track" roads are left out
    assert 0 < glob["f1b"] < 1 and set(glob) == set(M.GLOBAL_KEYS)


def test_metrics_equal_the_reference_formulas_in_pandas():
    pd = pytest.importorskip("pandas")
    rows, cats = _random_rows(11)
    df = pd.DataFrame([{"cover_type": r["cover_type"], "CATEGORY": cats[r["road_id"]]} for r in rows if cats[r["road_id"]] in CLASSES])
    df["tag"] = df.apply(lambda row: M.tag(row.cover_type, row.CATEGORY), axis=1)
    d = {"Pk": [], "Rk": [], "count": []}
    for k in CLASSES:
        tp = df[(df["tag"] == "TP") & (df["CATEGORY"] == k)].shape[0]
        fp = df[(df["tag"] == "wrong class") & (df["cover_type"] == k)].shape[0]
        fn = df[(df["tag"] == "wrong class") & (df["CATEGORY"] == k)].shape[0] + df[(df["tag"] == "FN") & (df["CATEGORY"] == k)].shape[0]
        d["Pk"].append(tp / (tp + fp) if tp else 0)
        d["Rk"].append(tp / (tp + fn) if tp else 0)
        d["count"].append(df[df["CATEGORY"] == k].shape[0])
    m = pd.DataFrame(d)
    total = m["count"].sum()
    pw, rw = (m["Pk"] * m["count"]).sum() / total, (m["Rk"] * m["count"]).sum() / total
    pb, rb = m["Pk"].sum() / 2, m["Rk"].sum() / 2
    by_class, glob = M.metrics(rows, cats, CLASSES)
    assert [c["Pk"] for c in by_class] == d["Pk"] and [c["Rk"] for c in by_class] == d["Rk"] and [c["count"] for c in by_class] == d["count"]
    assert (glob["Pw"], glob["Rw"], glob["Pb"], glob["Rb"]) == (pw, rw, pb, rb)
    assert glob["f1w"] == 2 * pw * rw / (pw + rw) and glob["f1b"] == 2 * pb * rb / (pb + rb)


def test_classes_without_a_true_positive_give_zeros():
    rows = [{"road_id": 0, "cover_type": "natural"}, {"road_id": 1, "cover_type": "undetected"}, {"road_id": 2, "cover_type": "undetermined"}]
    cats = {0: "artificial", 1: "artificial", 2: "natural"}
    by_class, glob = M.metrics(rows, cats, CLASSES)
    assert by_class == [{"cover_class": "artificial", "TP": 0, "FP": 0, "FN": 2, "Pk": 0, "Rk": 0, "f1k": 0, "count": 2},
                        {"cover_class": "natural", "TP": 0, "FP": 1, "FN": 1, "Pk": 0, "Rk": 0, "f1k": 0, "count": 1}]
    assert glob == {"Pw": 0, "Rw": 0, "f1w": 0, "Pb": 0, "Rb": 0, "f1b": 0}


def _g(*pairs):
    return [{"f1b": f, "Pb": p} for f, p in pairs]


def test_best_threshold_on_hand_written_sequences():
    thr = [0.0, 0.05, 0.1, 0.15000000000000002]
    assert M.best_threshold(thr, _g((0.5, 0.5), (0.6, 0.1), (0.7, 0.1), (0.65, 0.9))) == (2, 0.1)        # strictly better later
    assert M.best_threshold(thr, _g((0.5, 0.5), (0.5, 0.6), (0.4, 0.9), (0.5, 0.7))) == (3, 0.15)        # equal f1b, larger Pb replaces
    assert M.best_threshold(thr, _g((0.5, 0.5), (0.5, 0.5), (0.5, 0.4), (0.4, 0.9))) == (0, 0.0)         # equal f1b, equal or smaller Pb does not
    assert M.best_threshold(thr, _g((0.3, 0.3), (0.3, 0.3), (0.3, 0.3), (0.3, 0.3))) == (0, 0.0)         # all equal: the first
    assert M.best_threshold([0.3], _g((0.0, 0.0))) == (0, 0.3)
    with pytest.raises(ValueError):
        M.best_threshold(thr, _g((0.1, 0.1)))


def test_no_float32_score_lies_between_a_reference_threshold_and_its_rounding():
    thr = M.REFERENCE_THRESHOLDS
    assert thr.size == 20 and sum(float(t) != round(float(t), 2) for t in thr) == 7 and float(thr[3]) == 0.15000000000000002
    assert M.threshold_rounding_is_safe(thr)
    for t in thr:                                               # the same, spelled out on the float32 values around each
        t, r = float(t), round(float(t), 2)
        s = np.float32(t)
        for v in (np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(2))):
            assert (np.float64(v) >= t) == (np.float64(v) >= r), (t, v)
    assert not M.threshold_rounding_is_safe([float(np.float32(0.3)) + 1e-12])       # float32(0.3) lies between this and 0.3


def test_diff_sweep_accepts_only_strictly_larger():
    # four roads of category artificial; diff scores 0.02, 0.07, 0.5, 0.5.  f1b per threshold: covers wrong at low diff become FN
    rows = [{"road_id": 0, "cover_type": "natural", "diff_score": 0.02}, {"road_id": 1, "cover_type": "natural", "diff_score": 0.07},
            {"road_id": 2, "cover_type": "artificial", "diff_score": 0.5}, {"road_id": 3, "cover_type": "natural", "diff_score": 0.5}]
    cats = {0: "artificial", 1: "artificial", 2: "artificial", 3: "natural"}
    thr = [0.0, 0.05, 0.1, 0.6]
    got = M.diff_sweep(rows, cats, CLASSES, thr)
    f1 = [e["global"]["f1b"] for e in got["zones"]["all"]]
    want = []
    for t in thr:
        filtered = [dict(r, cover_type="undetermined" if r["diff_score"] < t else r["cover_type"]) for r in rows]
        want.append(_brute(filtered, cats, CLASSES)[1]["f1b"])
    assert f1 == want and f1[1] > f1[0] and f1[2] > f1[1] and f1[3] == 0
    assert got["best_index"] == 2 and got["best_threshold"] == 0.1
    flat = M.diff_sweep([dict(r, diff_score=1.0) for r in rows], cats, CLASSES, thr[:3])      # nothing changes: equal f1b never replaces
    assert flat["best_index"] == 0 and len({e["global"]["f1b"] for e in flat["zones"]["all"]}) == 1
    zoned = M.diff_sweep(rows, cats, CLASSES, thr, {"training zone": [0, 1, 2], "inference-only zone": [3]})
    assert [e["global"] for e in zoned["zones"]["inference-only zone"]][0] == M.metrics(rows[3:], cats, CLASSES)[1]
    assert zoned["best_index"] == M.diff_sweep(rows[:3], cats, CLASSES, thr)["best_index"]


def test_accuracy_and_baseline():
    rows, cats = _random_rows(3, n=40)
    acc = M.accuracy(rows, cats)
    n = len(rows)
    assert acc["right"] == sum(1 for r in rows if cats[r["road_id"]] == r["cover_type"]) / n * 100
    assert acc["undetected"] == sum(1 for r in rows if r["cover_type"] == "undetected") / n * 100
    assert acc["wrong"] == round(100 - acc["right"] - acc["undetected"] - acc["undetermined"], 2)
    assert M.baseline(rows, cats, CLASSES, "natural") == _brute([dict(r, cover_type="natural") for r in rows], cats, CLASSES)
    by_class, _ = M.baseline(rows, cats, CLASSES)
    assert by_class[0]["Rk"] == 1 and by_class[1]["TP"] == 0


# ---------------------------------------------------------------------------------------------------- end to end on the CPU
A, N = 0, 1                                                     # det_class of "artificial" / "natural" (raster_vote.CLASS_NAMES)
TRUTH = {"a": "artificial", "tie": "artificial", "none": "natural", "split": "natural", "wrong": "artificial", "b": "natural",
         "c": "natural", "d": "artificial"}


def _scene():
    """dataset -> tiles of (road ids, label areas, scores, classes, inter (labels, detections)).  `split` lies in both tiles of val;
    `none` meets nothing (undetected); `tie` has one pair per class of equal weight and score (undetermined); `wrong` is artificial
    in truth and has only two natural pairs, scoring 0.12 and 0.14: wrong class up to threshold 0.10, undetected -- no false
    positive of `natural` any more -- from 0.15 on."""
    f32 = lambda *v: np.array(v, np.float32)
    val0 = (["a", "tie", "none", "split", "wrong"], np.array([100, 100, 100, 200, 100]),
            f32(0.9, 0.6, 0.6, 0.55, 0.12, 0.14), np.array([A, N, A, N, N, N]),
            np.array([[60, 0, 0, 0, 0, 0], [0, 50, 50, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 0, 0, 80, 0, 0], [0, 0, 0, 0, 40, 30]]))
    val1 = (["split", "b"], np.array([300, 64]), f32(0.8, 0.3, 0.45), np.array([N, A, N]), np.array([[120, 31, 0], [0, 7, 64]]))
    tst0 = (["c", "d"], np.array([50, 80]), f32(0.7, 0.6, 0.3), np.array([N, A, N]), np.array([[50, 0, 0], [0, 60, 20]]))
    return {"val": [val0, val1], "tst": [tst0]}


def _row_route(tiles, threshold):
    rows = [r for ids, area, sc, cl, inter in tiles for r in RV.weighted_scores(inter, area, sc, cl, ids)]
    return RV.determine_detected_class(rows, [rid for t in tiles for rid in t[0]], threshold)


def _sweep_sets(thr):
    return {name: ([t[0] for t in tiles], [RV.votes_from_counts(t[4].T, t[1], t[2], t[3], 2, thresholds=thr) for t in tiles])
            for name, tiles in _scene().items()}


def test_the_whole_route_equals_the_row_route_per_threshold():
    thr = M.REFERENCE_THRESHOLDS
    scene, sets = _scene(), _sweep_sets(thr)
    doc = M.report(sets, TRUTH, CLASSES, thr)
    assert doc["thresholds"] == [float(t) for t in thr] and doc["sweep_on"] == "val" and len(doc["sweep"]) == 20
    covers_at = {}
    for j, t in enumerate(thr):
        want = _row_route(scene["val"], float(t))
        got = RV.reduce_votes([RV.sweep_slice(row + (None,), j) for row in sets["val"][1]], sets["val"][0])
        assert [w["road_id"] for w in want] == [g["road_id"] for g in got] == ["a", "tie", "none", "split", "wrong", "b"]
        for w, g in zip(want, got):
            assert w["cover_type"] == g["cover_type"], (j, w, g)
            for k in ("nat_score", "art_score", "diff_score"):
                assert abs(w[k] - g[k]) <= 1e-12, (j, k, w, g)
        by_class, glob = _brute(want, TRUTH, CLASSES)
        assert doc["sweep"][j] == {"threshold": float(t), "by_class": by_class, "global": glob}
        covers_at[j] = {g["road_id"]: g["cover_type"] for g in got}
    assert covers_at[0]["tie"] == "undetermined" and covers_at[0]["none"] == "undetected" and covers_at[0]["wrong"] == "natural"
    assert covers_at[2]["wrong"] == "natural" and covers_at[3]["wrong"] == "undetected"          # both pairs drop out at 0.15
    f1 = [s["global"]["f1b"] for s in doc["sweep"]]
    assert f1[3] > f1[0] and doc["best_index"] == 3 and doc["best_threshold"] == 0.15 != float(thr[3])
    assert (doc["best_index"], doc["best_threshold"]) == M.best_threshold(thr, [s["global"] for s in doc["sweep"]])
    # at the best threshold: every dataset from its own tiles only, the zones, and the unfiltered table
    assert list(doc["datasets"]) == ["all datasets", "val", "tst", "training zone", "all predictions without filter"]
    both = scene["val"] + scene["tst"]
    for name, tiles, t in (("all datasets", both, 0.15), ("val", scene["val"], 0.15), ("tst", scene["tst"], 0.15), ("training zone", both, 0.15),
                           ("all predictions without filter", both, 0.0)):
        by_class, glob = _brute(_row_route(tiles, t), TRUTH, CLASSES)
        assert doc["datasets"][name] == {"by_class": by_class, "global": glob}, name
    assert doc["datasets"]["tst"]["global"]["f1b"] == 1.0 and doc["datasets"]["all datasets"]["by_class"][0]["count"] == 4
    best_rows = _row_route(both, 0.15)
    assert doc["accuracy"] == M.accuracy(best_rows, TRUTH) and doc["accuracy"]["right"] == 5 / 8 * 100
    assert doc["baseline"]["class"] == "artificial" and doc["baseline"]["global"] == _brute([dict(r, cover_type="artificial") for r in best_rows], TRUTH, CLASSES)[1]
    assert list(doc["diff_sweep"]["zones"]) == ["training zone"] and len(doc["diff_sweep"]["zones"]["training zone"]) == 20
    import json
    assert json.loads(json.dumps(doc)) == doc                   # plain Python numbers throughout


def test_report_without_val_sweeps_all_roads_and_knows_the_oth_zone():
    thr = [0.3, 0.0]
    sets = _sweep_sets(thr)
    sets = {"trn": sets["val"], "oth": sets["tst"]}
    doc = M.report(sets, TRUTH, CLASSES, thr)
    assert doc["sweep_on"] == "all datasets" and list(doc["datasets"])[:5] == ["all datasets", "trn", "oth", "training zone", "inference-only zone"]
    assert doc["datasets"]["inference-only zone"] == doc["datasets"]["oth"] and doc["datasets"]["training zone"] == doc["datasets"]["trn"]
    assert list(doc["diff_sweep"]["zones"]) == ["training zone", "inference-only zone"]
    assert ("all predictions without filter" in doc["datasets"]) == (doc["best_threshold"] != 0)
