"""The reference's final metrics (R:scripts/road_segmentation/final_metrics.py) on the road tables ``raster_vote.reduce_votes`` gives:
the one number the reference publishes is the balanced F1 of the per-road cover classes at the best of 20 score thresholds.  Pure
Python and numpy.

A road table is a list of dicts with ``road_id`` and ``cover_type`` (``diff_score`` too, for ``diff_sweep``); ``categories`` maps a
road to its ground-truth category (the reference's CATEGORY column); ``classes`` is the reference's CLASSES (:235), in order.

    sweep  = Engine.road_votes_sweep / LanePipeline.run(..., vote_sweep=thresholds): per-(tile, label) tables of every threshold
    tables = [reduce_votes([sweep_slice(row, j) for row in tiles], road_ids) for j in range(T)]
    globals_ = [metrics(t, categories, classes)[1] for t in tables]                  (:280-293)
    j, best = best_threshold(thresholds, globals_)                                   (:295-309)
    metrics(tables[j], ...) per dataset, accuracy, diff_sweep, baseline              (:331-525)

NOT restated, on purpose: the random baseline (:504-509; it depends on the reference's row order through ``np.random.seed(0)``), the
reliability bins (:530 ff.; the reference's ``threshold-0.5`` makes them cumulative, and plotting is their only use), the plotly
output, and the quarry rule and the other GIS filters (:237-255), which belong to label preparation."""
from __future__ import annotations

import logging
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

log = logging.getLogger(__name__)
REFERENCE_THRESHOLDS = np.arange(0, 1., 0.05)          # R:final_metrics.py:277
GLOBAL_KEYS = ("Pw", "Rw", "f1w", "Pb", "Rb", "f1b")


def tag(cover, category) -> str:
    """``get_tag`` (R:final_metrics.py:91-105): a cover of "undetermined" or "undetected" is ``FN``; a cover equal to the category is
    ``TP``; anything else is ``wrong class``."""
    if cover == "undetermined" or cover == "undetected":
        return "FN"
    return "TP" if cover == category else "wrong class"


def metrics(rows: Sequence[Dict], categories: Dict, classes: Sequence[str]) -> Tuple[List[Dict], Dict]:
    """``get_metrics`` (R:final_metrics.py:33-89).  Per class k, in the order of ``classes``: TP = roads tagged TP of category k
    (:36-37); FP = roads tagged wrong class whose COVER is k (:38-39); FN = roads tagged FN of category k plus roads tagged wrong
    class of category k (:40-47); ``Pk = TP / (TP + FP)``, ``Rk = TP / (TP + FN)``, ``f1k = 2 Pk Rk / (Pk + Rk)``, all three 0 when
    TP is 0 (:49-56); ``count`` = roads of category k (:62).  Global: ``Pw = sum(Pk * count) / sum(count)`` and ``Rw`` likewise
    (:66-70; 0 when no road counts, where the reference would divide by zero), ``f1w`` 0 when both are 0, else
    ``2 Pw Rw / (Pw + Rw)`` (:72-75); ``Pb = sum(Pk) / len(classes)``, ``Rb`` likewise and ``f1b`` formed like ``f1w`` (:78-84) -- the
    reference divides by a literal 2, which is ``len(classes)`` for its two classes.  The sums are sequential float64 adds in class
    order.  Roads whose category is not among ``classes`` (or that ``categories`` does not know) are left out, as the reference's
    per-class filters leave them out, and counted in the log.  Returns (by-class rows, global dict)."""
    classes = list(classes)
    at = {k: i for i, k in enumerate(classes)}
    tp, fp, fn, count = ([0] * len(classes) for _ in range(4))
    left_out = 0
    for r in rows:
        cat = categories.get(r["road_id"])
        if cat not in at:
            left_out += 1
            continue
        k = at[cat]
        count[k] += 1
        what = tag(r["cover_type"], cat)
        if what == "TP":
            tp[k] += 1
        elif what == "FN":
            fn[k] += 1
        else:
            fn[k] += 1
            if r["cover_type"] in at:
                fp[at[r["cover_type"]]] += 1
    if left_out:
        log.info("road metrics: %d roads left out, their category is not among %s", left_out, classes)
    by_class = []
    for i, k in enumerate(classes):
        if tp[i] == 0:
            pk = rk = f1k = 0
        else:
            pk = tp[i] / (tp[i] + fp[i])
            rk = tp[i] / (tp[i] + fn[i])
            f1k = 2 * pk * rk / (pk + rk)
        by_class.append({"cover_class": k, "TP": tp[i], "FP": fp[i], "FN": fn[i], "Pk": pk, "Rk": rk, "f1k": f1k, "count": count[i]})
    total = sum(count)
    s_pw = s_rw = s_p = s_r = 0.0
    for c in by_class:
        s_pw = s_pw + c["Pk"] * c["count"]
        s_rw = s_rw + c["Rk"] * c["count"]
        s_p = s_p + c["Pk"]
        s_r = s_r + c["Rk"]
    pw, rw = (s_pw / total, s_rw / total) if total else (0.0, 0.0)
    pb, rb = s_p / len(classes), s_r / len(classes)
    f1 = lambda p, r: 0 if p == 0 and r == 0 else 2 * p * r / (p + r)
    return by_class, {"Pw": pw, "Rw": rw, "f1w": f1(pw, rw), "Pb": pb, "Rb": rb, "f1b": f1(pb, rb)}


def best_threshold(thresholds: Sequence[float], globals_: Sequence[Dict]) -> Tuple[int, float]:
    """The reference's chooser (R:final_metrics.py:295-309): the first entry starts as best; a later entry replaces it when its
    ``f1b`` is larger, or when its ``f1b`` is equal and its ``Pb`` is larger.  Returns (index, ``round(threshold, 2)``): the reference
    reports the rounded value and re-runs with it; the table to use is the sweep's slice at the index, which is the same table --
    no float32 score lies between one of ``np.arange(0, 1., 0.05)`` and its two-decimal rounding (``threshold_rounding_is_safe``).
    (The reference starts with ``threshold == 0``, its first entry.)"""
    if len(thresholds) != len(globals_) or not len(thresholds):
        raise ValueError(f"{len(globals_)} metric sets for {len(thresholds)} thresholds")
    best, max_f1, max_p = 0, globals_[0]["f1b"], globals_[0]["Pb"]
    for j in range(1, len(thresholds)):
        g = globals_[j]
        if g["f1b"] > max_f1 or (g["f1b"] == max_f1 and g["Pb"] > max_p):
            best, max_f1, max_p = j, g["f1b"], g["Pb"]
    return best, round(float(thresholds[best]), 2)


def threshold_rounding_is_safe(thresholds: Iterable[float]) -> bool:
    """Does ``score >= t`` equal ``score >= round(t, 2)`` for every float32 score?  True when no float32 value lies in the half-open
    interval between the two, whichever is smaller: checked on the float32 values next to both."""
    for t in thresholds:
        t, r = float(t), round(float(t), 2)
        lo, hi = min(t, r), max(t, r)
        near = np.float32(lo)
        for s in (np.nextafter(near, np.float32(-np.inf)), near, np.nextafter(near, np.float32(np.inf))):
            if lo <= float(s) < hi:
                return False
    return True


def accuracy(rows: Sequence[Dict], categories: Dict) -> Dict[str, float]:
    """The shares of the roads, in percent (R:final_metrics.py:393-401): ``right`` (cover equal to the category), ``undetected``,
    ``undetermined``, and ``wrong`` = round(100 - the three, 2) as the reference forms it; the first three are not rounded (the
    reference rounds them to 2 decimals only in its log)."""
    n = len(rows)
    if not n:
        return {"right": 0.0, "undetermined": 0.0, "undetected": 0.0, "wrong": 0.0}
    right = sum(1 for r in rows if categories.get(r["road_id"]) == r["cover_type"]) / n * 100
    missing = sum(1 for r in rows if r["cover_type"] == "undetected") / n * 100
    undetermined = sum(1 for r in rows if r["cover_type"] == "undetermined") / n * 100
    return {"right": right, "undetermined": undetermined, "undetected": missing, "wrong": round(100 - right - missing - undetermined, 2)}


def diff_sweep(rows: Sequence[Dict], categories: Dict, classes: Sequence[str], thresholds: Sequence[float],
               zones: Optional[Dict[str, Iterable]] = None) -> Dict:
    """The sweep on the difference between the two indices (R:final_metrics.py:429-478), on the table at the best score threshold:
    for each threshold the cover becomes "undetermined" where ``diff_score < threshold`` (:434), metrics are taken per zone
    (``zones``: name -> the zone's roads, the reference's gt_type 'gt' and 'oth', :437-456; None = one zone "all" of every road), and
    the chooser runs on the FIRST zone and accepts a strictly larger ``f1b`` only (:458-472), the first entry starting as best.
    Returns {"zones": {name: [{"threshold", "by_class", "global"}, ...]}, "best_index", "best_threshold" (rounded to 2 decimals)}."""
    zone_sets = {"all": None} if zones is None else {k: set(v) for k, v in zones.items()}
    out: Dict = {"zones": {k: [] for k in zone_sets}}
    best, max_f1 = 0, None
    for j, t in enumerate(thresholds):
        t = float(t)
        filtered = [dict(r, cover_type="undetermined") if r["diff_score"] < t else r for r in rows]
        for z, (name, ids) in enumerate(zone_sets.items()):
            mine = filtered if ids is None else [r for r in filtered if r["road_id"] in ids]
            by_class, glob = metrics(mine, categories, classes)
            out["zones"][name].append({"threshold": t, "by_class": by_class, "global": glob})
            if z == 0 and (max_f1 is None or glob["f1b"] > max_f1):
                best, max_f1 = j, glob["f1b"]
    out["best_index"] = best
    out["best_threshold"] = round(float(thresholds[best]), 2) if len(thresholds) else 0
    return out


def baseline(rows: Sequence[Dict], categories: Dict, classes: Sequence[str], cls: str = "artificial") -> Tuple[List[Dict], Dict]:
    """The metrics when every road is given the class ``cls`` (R:final_metrics.py:499-502, :515-518)."""
    return metrics([dict(r, cover_type=cls) for r in rows], categories, classes)


def report(datasets: Dict[str, Tuple[Sequence[Sequence], Sequence[Sequence[np.ndarray]]]], categories: Dict, classes: Sequence[str],
           thresholds: Sequence[float], class_names=None, baseline_class: str = "artificial") -> Dict:
    """The document ``make_detections --road-metrics`` writes, from the sweep tables of every dataset: datasets[name] = (road ids per
    tile, sweep tables per tile ``(wscore (T, L, K), wfrac, pairs, ...)``), in dataset order and tile order.  A road table of a set of
    datasets at threshold j is ``reduce_votes`` of slice j of those datasets' tiles -- each road's pieces come only from those
    datasets, summed in dataset order, then tile order.
      thresholds      the list
      sweep           per threshold, by-class and global metrics of the dataset ``val`` (:270-293); without one, of all roads
                      (``sweep_on`` says which)
      best_threshold  ``best_threshold``; ``best_index`` beside it
      datasets        at the best threshold (:331-383): "all datasets", every single dataset, "training zone" (every dataset but
                      ``oth``), "inference-only zone" (``oth``, where present), and "all predictions without filter" -- the slice of
                      threshold 0 -- where the best threshold is not 0 and the list holds a 0
      accuracy, diff_sweep (zones as above; its chooser runs on the training zone), baseline: on the table of all datasets."""
    from .raster_vote import CLASS_NAMES, reduce_votes
    names = CLASS_NAMES if class_names is None else class_names
    thr = [float(t) for t in thresholds]

    def table(which: Sequence[str], j: int) -> List[Dict]:
        return reduce_votes([(t[0][j], t[1][j], t[2][j]) for d in which for t in datasets[d][1]], [ids for d in which for ids in datasets[d][0]], names)

    def entry(rows: List[Dict]) -> Dict:
        by_class, glob = metrics(rows, categories, classes)
        return {"by_class": by_class, "global": glob}
    every = list(datasets)
    sweep_on = ["val"] if "val" in datasets else every
    if "val" not in datasets:
        log.info("road metrics: no dataset named 'val', the threshold sweep runs over all roads")
    sweep = [dict(threshold=t, **entry(table(sweep_on, j))) for j, t in enumerate(thr)]
    best, best_thr = best_threshold(thr, [s["global"] for s in sweep])
    all_rows = table(every, best)
    training = [d for d in every if d != "oth"]
    per = {"all datasets": entry(all_rows)}
    for d in every:
        per[d] = entry(table([d], best))
    per["training zone"] = entry(table(training, best))
    if "oth" in datasets:
        per["inference-only zone"] = entry(table(["oth"], best))
    if best_thr != 0:
        if 0.0 in thr:
            per["all predictions without filter"] = entry(table(every, thr.index(0.0)))
        else:
            log.info("road metrics: no threshold 0 in the list, 'all predictions without filter' is left out")
    zones = {"training zone": {rid for d in training for ids in datasets[d][0] for rid in ids}}
    if "oth" in datasets:
        zones["inference-only zone"] = {rid for ids in datasets["oth"][0] for rid in ids}
    base_class, base_global = baseline(all_rows, categories, classes, baseline_class)
    return {"thresholds": thr, "sweep_on": "val" if "val" in datasets else "all datasets", "sweep": sweep, "best_index": best,
            "best_threshold": best_thr, "datasets": per, "accuracy": accuracy(all_rows, categories),
            "diff_sweep": diff_sweep(all_rows, categories, classes, thr, zones),
            "baseline": {"class": baseline_class, "by_class": base_class, "global": base_global}}
