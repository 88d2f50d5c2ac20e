"""Raster voting on the tile grid: the class vote of the reference's post-stage computed from the detection
MASKS instead of from vectorised polygons.

Reference (vector form, geopandas/shapely): ``determine_class.get_weighted_scores`` overlays the tile-clipped road labels with the
detection polygons, weights every (road, detection) intersection by ``round(area(intersection) / area(label), 2)``, keeps pairs
above 0.05, and ``determine_detected_class`` sums, per road and class, weighted scores over weights
(R:scripts/road_segmentation/determine_class.py:97-120, :122-190).  Here the intersection areas are pixel counts:
``|label_raster AND detection_mask|`` on the device (``rs_op_mask_overlap`` / ``rs_engine_label_overlap``: popcounts of bit-packed
rows, the detection masks never leave HBM), everything after the counts is restated line by line on the host.

Differences from the vector form, by construction: areas are counted in whole pixels of the tile grid (0.4 m at z18,
R:config/config_obj_detec.yaml:20,45), and RDP simplification (ε 0.75 px) does not enter.  The numpy statement of the device kernel (the
oracle of its test) is ``oracle/host_tail_oracle.py::overlap_counts``.

The streamed form (second half of this module) runs the whole vote behind the engine's forward: road labels as polygons in
tile pixels, rasterised and counted on the device, the per-(tile, label, class) sums formed by ``road_vote_kernel`` (csrc/road_vote.h), and
only those tables travel (``Engine.road_votes``, ``LanePipeline.run(..., labels=...)``).  ``vote_tables_host`` is the numpy route to the
same tables from fetched masks, ``reduce_votes`` the vectorised step from the tables of all tiles to the road table.  The sweep
(``Engine.road_votes_sweep``, ``road_votes_sweep_host / _device``, ``thresholds=`` of the numpy route) forms the tables of up to 32 score
thresholds in one pass, slice j with the bits of the tables at ``thresholds[j]``; ``road_metrics.py`` turns them into the reference's
final metrics."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Sequence, Tuple

import numpy as np

CLASS_NAMES = {0: "artificial", 1: "natural"}          # R:scripts/road_segmentation/determine_class.py:19-28 (det_class -> name)


def label_rasters(label_polygons: Sequence[Sequence[np.ndarray]], h: int, w: int) -> np.ndarray:
    """Bit-packed (n_labels, h, ceil(w/8)) rasters of road labels given as polygons in TILE PIXEL coordinates (one list of
    [x0, y0, x1, y1, ...] rings per label), pixel centres inside = 1 (the rasteriser of the training targets, square tiles)."""
    from .train_targets import rasterize_polygons_within_box
    if h != w:
        raise ValueError("label rasters are built for square tiles")
    out = np.zeros((len(label_polygons), h, (w + 7) // 8), np.uint8)
    for i, polys in enumerate(label_polygons):
        m = rasterize_polygons_within_box(polys, np.array([0.0, 0.0, float(w), float(h)]), h)
        out[i] = np.packbits(m, axis=1, bitorder="little")
    return out


def overlap_counts_device(lib, det_dev_ptr: int, n_det: int, lab_packed: np.ndarray, h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    """Counts for detection masks ALREADY on the device (``Engine.tensor_ptr("masks")`` + tile offset): uploads the label rasters,
    runs the kernel, reads the two small count arrays back."""
    import torch
    lab = torch.from_numpy(np.ascontiguousarray(lab_packed)).cuda()
    inter = torch.zeros((lab_packed.shape[0], n_det), dtype=torch.int32, device="cuda")
    area = torch.zeros((lab_packed.shape[0],), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib.rs_op_mask_overlap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = lib.rs_op_mask_overlap(C.c_void_p(det_dev_ptr), n_det, C.c_void_p(lab.data_ptr()), lab_packed.shape[0], h, w,
                                C.c_void_p(inter.data_ptr()), C.c_void_p(area.data_ptr()), None)
    if rc != 0:
        raise RuntimeError(f"rs_op_mask_overlap failed ({rc}): {lib.rs_last_error().decode(errors='replace')}")
    torch.cuda.synchronize()
    return inter.cpu().numpy(), area.cpu().numpy()


def pair_counts_device(det_packed: np.ndarray, det_count: np.ndarray, gt_packed: np.ndarray, tile_first: np.ndarray, side: int,
                       gt_cap: int = 128, prefill: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``rs_op_mask_pair_counts`` on host arrays (uploaded through torch): det_packed (tiles, slots, side, ceil(side / 8)) and gt_packed
    (instances, side, ceil(side / 8)) bit-packed masks, det_count (tiles,), tile_first (tiles + 1,) -> inter (tiles, slots, gt_cap),
    det_area (tiles, slots), gt_area (tiles, gt_cap) int32; everything outside the counted slots and the tiles' own ground truths is
    zero.  ``prefill``: what the output buffers hold before the call (the operator clears them itself)."""
    import torch
    from .engine import _check, load_library
    lib = load_library()
    n, slots = int(det_packed.shape[0]), int(det_packed.shape[1])
    dev = torch.device("cuda")
    det = torch.from_numpy(np.ascontiguousarray(det_packed)).to(dev)
    gt = torch.from_numpy(np.ascontiguousarray(gt_packed)).to(dev) if gt_packed.size else None
    cnt = torch.from_numpy(np.ascontiguousarray(det_count, np.int32)).to(dev)
    first = torch.from_numpy(np.ascontiguousarray(tile_first, np.int32)).to(dev)
    inter = torch.full((n, slots, gt_cap), prefill, dtype=torch.int32, device=dev)
    d_area = torch.full((n, slots), prefill, dtype=torch.int32, device=dev)
    g_area = torch.full((n, gt_cap), prefill, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_mask_pair_counts(det.data_ptr(), cnt.data_ptr(), n, slots, gt.data_ptr() if gt is not None else None, first.data_ptr(),
                                           gt_cap, side, inter.data_ptr(), d_area.data_ptr(), g_area.data_ptr(), None), "rs_op_mask_pair_counts")
    torch.cuda.synchronize()
    return inter.cpu().numpy(), d_area.cpu().numpy(), g_area.cpu().numpy()


def weighted_scores(inter: np.ndarray, label_area: np.ndarray, scores: np.ndarray, classes: np.ndarray, road_ids: Sequence) -> List[Dict]:
    """``get_weighted_scores`` (R:determine_class.py:97-120) from pixel counts: one row per (label, detection) pair with
    ``area_pred_in_label = round(intersection / label area, 2) > 0.05``; ``weighted_score = area_pred_in_label * score``."""
    rows = []
    for li in range(inter.shape[0]):
        if label_area[li] <= 0:
            continue
        for di in range(inter.shape[1]):
            if inter[li, di] <= 0:
                continue
            frac = float(np.round(inter[li, di] / label_area[li], 2))
            if frac > 0.05:
                rows.append({"OBJECTID": road_ids[li], "det": di, "score": float(scores[di]), "det_class": int(classes[di]),
                             "det_class_name": CLASS_NAMES.get(int(classes[di]), str(int(classes[di]))),
                             "area_pred_in_label": frac, "weighted_score": frac * float(scores[di])})
    return rows


def determine_detected_class(rows: Sequence[Dict], road_ids: Sequence, threshold: float = 0.0) -> List[Dict]:
    """``determine_detected_class`` (R:determine_class.py:122-190): per road, the class whose score-weighted mean
    (sum of weighted scores / sum of weights over the road's pairs with score >= threshold) is larger; "undetected" without
    pairs, "undetermined" on a tie; scores rounded to 3 decimals, ``diff_score`` their absolute difference."""
    valid = [r for r in rows if r["score"] >= threshold]
    out = []
    seen = []
    for rid in road_ids:
        if rid in seen:
            continue
        seen.append(rid)
        mine = [r for r in valid if r["OBJECTID"] == rid]
        if not mine:
            out.append({"road_id": rid, "cover_type": "undetected", "nat_score": 0, "art_score": 0, "diff_score": 0})
            continue
        idx = {}
        for name in ("natural", "artificial"):
            ws = sum(r["weighted_score"] for r in mine if r["det_class_name"] == name)
            wa = sum(r["area_pred_in_label"] for r in mine if r["det_class_name"] == name)
            idx[name] = 0 if ws == 0 else ws / wa
        nat, art = idx["natural"], idx["artificial"]
        cover = "undetermined" if art == nat else ("artificial" if art > nat else "natural")
        out.append({"road_id": rid, "cover_type": cover, "nat_score": round(nat, 3), "art_score": round(art, 3),
                    "diff_score": 0 if art == nat else abs(art - nat)})
    return out


# ---------------------------------------------------------------------------------------------------- the streamed form
# csrc/road_vote.h states the vote as a rule per (tile, label, class) cell; ``rs_op_road_votes`` / ``rs_engine_fetch_votes_async`` run
# it on the device behind the forward, ``rs_host_road_votes`` and ``vote_tables_host`` on the host.  ``reduce_votes`` is the step
# from the per-(tile, label) tables to the road table.
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)
TABLE_KEYS = ("det_scores", "det_classes", "det_count", "tile_first", "inter", "gt_area")


def sweep_thresholds(thresholds) -> np.ndarray:
    """A threshold list as the sweep takes it (csrc/road_vote.h, THE SWEEP): 1 to 32 finite float64 values, in any order."""
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
    if not 1 <= thr.size <= 32 or not np.isfinite(thr).all():
        raise ValueError(f"a vote sweep takes 1 to 32 finite thresholds, got {thr.tolist()!r}")
    return thr


def votes_from_counts(inter: np.ndarray, label_area: np.ndarray, scores: np.ndarray, classes: np.ndarray, num_classes: int,
                      threshold: float = 0.0, thresholds=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The rule of csrc/road_vote.h on one tile's counts in numpy: inter (D, L) and label_area (L,) pixel counts, scores / classes
    (D,) -> wscore, wfrac (L, K) float64 and pairs (L, K) int32.  The detections are walked in ascending order, so every cell is the
    sequential float64 sum the kernel forms.  ``thresholds=`` (a list, ``threshold`` is then not read): the sweep, tables of shape
    (T, L, K) whose slice j is this function at ``thresholds[j]``."""
    if thresholds is not None:
        per = [votes_from_counts(inter, label_area, scores, classes, num_classes, float(t)) for t in sweep_thresholds(thresholds)]
        return tuple(np.stack([p[i] for p in per]) for i in range(3))
    L, K = int(label_area.shape[0]), int(num_classes)
    ws, wa, pairs = np.zeros((L, K)), np.zeros((L, K)), np.zeros((L, K), np.int32)
    area = np.asarray(label_area, np.int64)
    ok = area > 0
    for d in range(int(scores.shape[0])):
        c, s = int(classes[d]), float(scores[d])
        if not 0 <= c < K or not s >= threshold:
            continue
        i = np.asarray(inter[d], np.int64)
        frac = np.zeros(L)
        frac[ok] = np.round(i[ok] / area[ok], 2)
        keep = ok & (i > 0) & (frac > 0.05)
        ws[keep, c] += frac[keep] * s
        wa[keep, c] += frac[keep]
        pairs[keep, c] += 1
    return ws, wa, pairs


def vote_tables_host(instances: Sequence, labels: Sequence[Sequence[Sequence[np.ndarray]]], num_classes: int,
                     threshold: float = 0.0, thresholds=None) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """The numpy route to the tables ``Engine.road_votes`` gives, from fetched masks: per tile, ``label_rasters`` of labels[tile] (lists
    of rings in tile pixels), popcounts of the packed label AND the packed detection masks of instances[tile] (``Instances`` with
    masks), then ``votes_from_counts``.  Returns per tile ``(wscore (L, K), wfrac (L, K), pairs (L, K), label_area (L,))``.  The
    fallback of a batch that does not fit the device pool.  ``thresholds=``: the sweep (``Engine.road_votes_sweep``), the three
    tables then have the shape (T, L, K); rasters and counts are formed once."""
    if len(instances) != len(labels):
        raise ValueError(f"{len(labels)} label lists for {len(instances)} tiles")
    out = []
    for inst, labs in zip(instances, labels):
        h, w = inst.image_size
        det = inst._packed
        if det is None:
            raise ValueError("the host vote needs the detections' masks (MASK_ON, and a fetch that brings them)")
        lab = label_rasters(labs, h, w)
        inter = np.zeros((len(inst), len(labs)), np.int32)
        for g in range(len(labs)):
            inter[:, g] = _POP8[det & lab[g][None]].sum(axis=(1, 2), dtype=np.int64)
        area = _POP8[lab].sum(axis=(1, 2), dtype=np.int64).astype(np.int32) if len(labs) else np.zeros(0, np.int32)
        out.append(votes_from_counts(inter, area, inst.scores, inst.pred_classes, num_classes, threshold, thresholds) + (area,))
    return out


def _vote_call(entry: str, b: Dict[str, np.ndarray], num_classes: int, threshold: float, prefill: float, device: bool):
    from .engine import _check, load_library
    lib = load_library()
    n, slots = b["det_scores"].shape
    cap = int(b["gt_area"].shape[1])
    tabs = [np.ascontiguousarray(b["det_scores"], np.float32), np.ascontiguousarray(b["det_classes"], np.int32),
            np.ascontiguousarray(b["det_count"], np.int32), np.ascontiguousarray(b["tile_first"], np.int32),
            np.ascontiguousarray(b["inter"], np.int32), np.ascontiguousarray(b["gt_area"], np.int32)]
    outs = [np.full((n, cap, num_classes), prefill, np.float64), np.full((n, cap, num_classes), prefill, np.float64),
            np.full((n, cap, num_classes), int(prefill), np.int32)]
    if not device:
        _check(lib, lib.rs_host_road_votes(*[a.ctypes.data for a in tabs], n, num_classes, slots, cap, float(threshold),
                                           *[a.ctypes.data for a in outs]), entry)
        return tuple(outs)
    import torch
    dev = [torch.from_numpy(a).cuda() for a in tabs + outs]
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_road_votes(*[a.data_ptr() for a in dev[:6]], n, num_classes, slots, cap, float(threshold),
                                     *[a.data_ptr() for a in dev[6:]], None), entry)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in dev[6:])


def road_votes_host(b: Dict[str, np.ndarray], num_classes: int, threshold: float = 0.0, prefill: float = 0.0):
    """``rs_host_road_votes`` on a dict of the tables ``TABLE_KEYS`` (det_scores / det_classes (n, slots), det_count (n,), tile_first
    (n + 1,), inter (n, slots, gt_cap), gt_area (n, gt_cap)) -> wscore, wfrac (n, gt_cap, K) float64, pairs (n, gt_cap, K) int32.
    ``prefill``: what the output buffers hold before the call (the entry clears them itself).  Needs no device."""
    return _vote_call("rs_host_road_votes", b, num_classes, threshold, prefill, False)


def road_votes_device(b: Dict[str, np.ndarray], num_classes: int, threshold: float = 0.0, prefill: float = 0.0):
    """``rs_op_road_votes`` on the same dict, uploaded through torch: the kernel's tables."""
    return _vote_call("rs_op_road_votes", b, num_classes, threshold, prefill, True)


def _vote_sweep_call(entry: str, b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float, device: bool):
    from .engine import _check, load_library
    lib = load_library()
    n, slots = b["det_scores"].shape
    cap = int(b["gt_area"].shape[1])
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)      # unchecked: the entry refuses a bad list itself
    T = int(thr.size)
    tabs = [np.ascontiguousarray(b["det_scores"], np.float32), np.ascontiguousarray(b["det_classes"], np.int32),
            np.ascontiguousarray(b["det_count"], np.int32), np.ascontiguousarray(b["tile_first"], np.int32),
            np.ascontiguousarray(b["inter"], np.int32), np.ascontiguousarray(b["gt_area"], np.int32)]
    shape = (n, max(T, 1), cap, num_classes)
    outs = [np.full(shape, prefill, np.float64), np.full(shape, prefill, np.float64), np.full(shape, int(prefill), np.int32)]
    if not device:
        _check(lib, lib.rs_host_road_votes_sweep(*[a.ctypes.data for a in tabs], n, num_classes, slots, cap, thr.ctypes.data, T,
                                                 *[a.ctypes.data for a in outs]), entry)
        return tuple(outs)
    import torch
    dev = [torch.from_numpy(a).cuda() for a in tabs + outs]
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_road_votes_sweep(*[a.data_ptr() for a in dev[:6]], n, num_classes, slots, cap, thr.ctypes.data, T,
                                           *[a.data_ptr() for a in dev[6:]], None), entry)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in dev[6:])


def road_votes_sweep_host(b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float = 0.0):
    """``rs_host_road_votes_sweep`` on the dict of ``road_votes_host`` and a threshold list (1 to 32 finite values) -> wscore, wfrac
    (n, T, gt_cap, K) float64, pairs (n, T, gt_cap, K) int32; slice ``[:, j]`` has the bits of ``road_votes_host`` at
    ``thresholds[j]``.  ``prefill`` as there.  Needs no device."""
    return _vote_sweep_call("rs_host_road_votes_sweep", b, num_classes, thresholds, prefill, False)


def road_votes_sweep_device(b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float = 0.0):
    """``rs_op_road_votes_sweep`` on the same dict, uploaded through torch: ``road_vote_sweep_kernel``'s tables."""
    return _vote_sweep_call("rs_op_road_votes_sweep", b, num_classes, thresholds, prefill, True)


def sweep_slice(row: Sequence[np.ndarray], j: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """Slice j of one tile's sweep tables ``(wscore (T, L, K), wfrac, pairs, label_area)``: the tile's single-threshold tables at
    ``thresholds[j]``, as ``reduce_votes`` takes them."""
    return row[0][j], row[1][j], row[2][j], row[3]


def reduce_votes(tables: Sequence[Sequence[np.ndarray]], road_ids: Sequence[Sequence], class_names: Dict[int, str] = CLASS_NAMES,
                 ndigits: int = 3) -> List[Dict]:
    """From the per-(tile, label) vote tables to the road table.  tables[tile] = (wscore (L, K), wfrac (L, K), pairs (L, K), ...) as
    ``Engine.road_votes`` / ``vote_tables_host`` give them (a leading ``Instances`` and a trailing label_area are ignored), road_ids[tile]
    = the road of each of the tile's labels.  A road's pieces -- its labels over all tiles -- are summed per class in (tile index, label
    index) order with sequential float64 adds, then ``index = 0 if ws == 0 else ws / wa`` and the cover rule of
    ``determine_detected_class``: "undetected" for a road without pairs, "undetermined" on a tie, scores rounded to ``ndigits``.  With
    the reference's two classes the dicts carry its keys (road_id, cover_type, nat_score, art_score, diff_score); with another class
    list one ``<name>_score`` per class, the unique maximum as the cover and ``diff_score`` = best minus second.  Roads come in order
    of first appearance.  Linear in labels and roads."""
    names = [class_names.get(c, str(c)) for c in range(len(class_names))] if isinstance(class_names, dict) else list(class_names)
    K = len(names)
    if len(tables) != len(road_ids):
        raise ValueError(f"{len(road_ids)} road id lists for {len(tables)} tiles")
    index: Dict = {}
    rows, ws_all, wa_all, pairs_all = [], [], [], []
    for t, ids in zip(tables, road_ids):
        t = [a for a in t if isinstance(a, np.ndarray) and a.ndim == 2]
        if len(t) != 3 or any(a.shape != (len(ids), K) for a in t):
            raise ValueError(f"a tile's vote tables must be three ({len(ids)}, {K}) arrays")
        rows.extend(index.setdefault(rid, len(index)) for rid in ids)
        ws_all.append(t[0]); wa_all.append(t[1]); pairs_all.append(t[2])
    R = len(index)
    ws, wa, pairs = np.zeros((R, K)), np.zeros((R, K)), np.zeros((R, K), np.int64)
    if rows:
        at = np.asarray(rows, np.int64)
        np.add.at(ws, at, np.concatenate(ws_all))          # unbuffered: one add per piece, in (tile, label) order
        np.add.at(wa, at, np.concatenate(wa_all))
        np.add.at(pairs, at, np.concatenate(pairs_all))
    reference = sorted(names) == ["artificial", "natural"]
    out = []
    for rid, r in index.items():
        if not pairs[r].any():
            zero = {"nat_score": 0, "art_score": 0} if reference else {f"{nm}_score": 0 for nm in names}
            out.append({"road_id": rid, "cover_type": "undetected", **zero, "diff_score": 0})
            continue
        idx = [0 if ws[r, c] == 0 else float(ws[r, c] / wa[r, c]) for c in range(K)]
        if reference:
            nat, art = idx[names.index("natural")], idx[names.index("artificial")]
            cover = "undetermined" if art == nat else ("artificial" if art > nat else "natural")
            out.append({"road_id": rid, "cover_type": cover, "nat_score": round(nat, ndigits), "art_score": round(art, ndigits),
                        "diff_score": 0 if art == nat else abs(art - nat)})
            continue
        order = sorted(range(K), key=lambda c: -idx[c])
        best, second = idx[order[0]], (idx[order[1]] if K > 1 else 0)
        unique = K == 1 or best > second
        out.append({"road_id": rid, "cover_type": names[order[0]] if unique else "undetermined",
                    **{f"{nm}_score": round(idx[c], ndigits) for c, nm in enumerate(names)}, "diff_score": best - second if unique else 0})
    return out


# ---------------------------------------------------------------------------------------------------- the polygon geometry
# csrc/poly_overlap.h states the weight of a (label, detection) pair on POLYGONS, as the reference's overlay takes it: the area of
# the intersection of the label's rings with the detection's (simplified) polygons over the label's area, rounded to two decimals.
# ``rs_op_polygon_overlaps`` / ``rs_engine_fetch_votes_poly_async`` compute it on the device from the polygoniser's vertex tables,
# ``rs_host_polygon_overlaps`` is the host restatement with the same bits; ``rs_*_road_votes_area_sweep`` is the vote's walk on those
# weights.  A label's rings are all exteriors, taken as simple and pairwise interior-disjoint (the pixel geometry above takes their
# union); overlapping label rings and labels with holes are not covered, and nothing checks for them.
POLY_TABLE_KEYS = ("header", "poly_ring_count", "ring_len", "xy", "det_count", "tile_first", "inst_first", "poly_off", "poly_len", "polys")
VOTE_GEOMETRIES = ("pixels", "polygons")


def check_vote_geometry(geometry: str, vectorize: str = "device") -> str:
    """``geometry`` as the vote entries take it; "polygons" reads the device polygoniser's tables, so it needs ``vectorize="device"``."""
    if geometry not in VOTE_GEOMETRIES:
        raise ValueError(f"vote geometry {geometry!r}: one of {VOTE_GEOMETRIES}")
    if geometry == "polygons" and vectorize != "device":
        raise ValueError("the vote geometry 'polygons' reads the device polygoniser's vertex tables: it needs vectorize='device'")
    return geometry


def pack_label_pool(labels: Sequence[Sequence[Sequence[np.ndarray]]]) -> Dict[str, np.ndarray]:
    """labels[tile][label] = list of rings ([x0, y0, x1, y1, ...], tile pixels) -> the packed tables the polygon entries read:
    tile_first (n + 1,), inst_first (labels + 1,), poly_off / poly_len (rings,) int32 in doubles, polys float64."""
    arrs = [np.asarray(r, np.float64).reshape(-1) for tile in labels for lab in tile for r in lab]
    lens = np.array([a.size for a in arrs] or [0], np.int32)
    if any(int(k) < 2 or int(k) & 1 for k in lens[:len(arrs)]):
        raise ValueError("a label ring is a flat list of x, y pairs")
    off = np.zeros(max(len(arrs), 1), np.int32)
    if len(arrs) > 1:
        off[1:] = np.cumsum(lens[:-1])
    inst_first = np.zeros(sum(len(t) for t in labels) + 1, np.int32)
    inst_first[1:] = np.cumsum([len(lab) for t in labels for lab in t])
    tile_first = np.zeros(len(labels) + 1, np.int32)
    tile_first[1:] = np.cumsum([len(t) for t in labels])
    return {"tile_first": tile_first, "inst_first": inst_first, "poly_off": off, "poly_len": lens,
            "polys": np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(1)}


def stack_polygon_tables(tables: Sequence, slots: int = 0) -> Dict[str, np.ndarray]:
    """``engine.PolygonTables`` of n tiles (offsets local to each) -> the batch form the polygoniser leaves on the device: header
    (n, slots, 8) with offsets into the concatenated poly_ring_count / ring_len / xy, and det_count (n,).  ``slots`` 0: the largest
    tile's count (at least 1)."""
    n = len(tables)
    D = max([int(slots), 1] + [int(t.header.shape[0]) for t in tables])
    header = np.zeros((n, D, 8), np.int32)
    base = np.zeros(3, np.int64)
    for i, t in enumerate(tables):
        c = int(t.header.shape[0])
        header[i, :c] = t.header
        header[i, :c, 4:7] += base.astype(np.int32)
        base += (len(t.poly_ring_count), len(t.ring_len), len(t.xy))
    return {"header": header, "poly_ring_count": np.ascontiguousarray(np.concatenate([t.poly_ring_count for t in tables] + [np.zeros(1, np.int32)])),
            "ring_len": np.ascontiguousarray(np.concatenate([t.ring_len for t in tables] + [np.zeros(1, np.int32)])),
            "xy": np.ascontiguousarray(np.concatenate([t.xy for t in tables] + [np.zeros((1, 2), np.int16)])),
            "det_count": np.array([int(t.header.shape[0]) for t in tables], np.int32)}


def polygon_tables_from_lists(polygons: Sequence[Sequence[Sequence[Sequence[Tuple[float, float]]]]], rdp_epsilon: float = 0.0):
    """Nested polygon lists of one tile (per instance a list of polygons, each a list of closed rings of (x, y), the exterior first:
    the form ``vectorize.vectorize_masks_native`` returns) -> ``engine.PolygonTables`` without a flagged instance.  The vertices are
    pixel corners: integers, kept as int16."""
    from .engine import POLY_HDR, PolygonTables
    hdr = np.zeros((len(polygons), POLY_HDR), np.int32)
    prc: List[int] = []
    rlen: List[int] = []
    xy: List[Tuple[int, int]] = []
    for i, polys in enumerate(polygons):
        hdr[i, 4:7] = (len(prc), len(rlen), len(xy))
        for rings in polys:
            prc.append(len(rings))
            for ring in rings:
                rlen.append(len(ring))
                for x, y in ring:
                    if x != int(x) or y != int(y) or not -32768 <= x <= 32767 or not -32768 <= y <= 32767:
                        raise ValueError(f"detection vertex ({x!r}, {y!r}) is no int16 pixel corner")
                    xy.append((int(x), int(y)))
        hdr[i, 1:4] = (len(prc) - hdr[i, 4], len(rlen) - hdr[i, 5], len(xy) - hdr[i, 6])
    return PolygonTables(hdr, np.array(prc, np.int32), np.array(rlen, np.int32), np.array(xy, np.int16).reshape(-1, 2), rdp_epsilon)


def _overlap_call(entry: str, b: Dict[str, np.ndarray], gt_cap: int, prefill: float, device: bool, raw_areas: bool = False):
    from .engine import _check, load_library
    lib = load_library()
    n, slots = b["header"].shape[:2]
    dts = (np.int32, np.int32, np.int32, np.int16, np.int32, np.int32, np.int32, np.int32, np.int32, np.float64)
    tabs = [np.ascontiguousarray(b[k], dt) for k, dt in zip(POLY_TABLE_KEYS, dts)]
    outs = [np.full((n, slots, gt_cap), prefill, np.float64), np.full((n, gt_cap), prefill, np.float64), np.full((n,), int(prefill), np.int32)]
    vp = C.c_void_p
    if not device:
        f = lib.rs_host_polygon_overlaps
        f.argtypes = [vp] * 10 + [C.c_int] * 4 + [vp] * 3
        _check(lib, f(*[a.ctypes.data for a in tabs], n, slots, gt_cap, int(raw_areas), *[a.ctypes.data for a in outs]), entry)
        return tuple(outs)
    import torch
    dev = [torch.from_numpy(a).cuda() for a in tabs + outs]
    torch.cuda.synchronize()
    f = lib.rs_op_polygon_overlaps
    f.argtypes = [vp] * 10 + [C.c_int] * 4 + [vp] * 4
    _check(lib, f(*[a.data_ptr() for a in dev[:10]], n, slots, gt_cap, int(raw_areas), *[a.data_ptr() for a in dev[10:]], None), entry)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in dev[10:])


def polygon_overlaps_host(b: Dict[str, np.ndarray], gt_cap: int = 128, prefill: float = 0.0, raw_areas: bool = False):
    """``rs_host_polygon_overlaps`` on a dict of the tables ``POLY_TABLE_KEYS`` (``stack_polygon_tables`` and ``pack_label_pool``
    give them) -> frac (n, slots, gt_cap) float64, label_area (n, gt_cap) float64, flagged (n,) int32.  ``prefill``: what the output
    buffers hold before the call (the entry clears them itself); ``raw_areas``: ``frac`` holds the computed areas, not the rounded
    weights.  Needs no device."""
    return _overlap_call("rs_host_polygon_overlaps", b, gt_cap, prefill, False, raw_areas)


def polygon_overlaps_device(b: Dict[str, np.ndarray], gt_cap: int = 128, prefill: float = 0.0, raw_areas: bool = False):
    """``rs_op_polygon_overlaps`` on the same dict, uploaded through torch: ``poly_overlap_kernel``'s tables."""
    return _overlap_call("rs_op_polygon_overlaps", b, gt_cap, prefill, True, raw_areas)


def _area_sweep_call(entry: str, b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float, device: bool):
    from .engine import _check, load_library
    lib = load_library()
    n, slots = b["det_scores"].shape
    cap = int(b["frac"].shape[2])
    thr = np.ascontiguousarray(thresholds, np.float64).reshape(-1)      # unchecked: the entry refuses a bad list itself
    T = int(thr.size)
    tabs = [np.ascontiguousarray(b["det_scores"], np.float32), np.ascontiguousarray(b["det_classes"], np.int32),
            np.ascontiguousarray(b["det_count"], np.int32), np.ascontiguousarray(b["tile_first"], np.int32),
            np.ascontiguousarray(b["frac"], np.float64)]
    shape = (n, max(T, 1), cap, num_classes)
    outs = [np.full(shape, prefill, np.float64), np.full(shape, prefill, np.float64), np.full(shape, int(prefill), np.int32)]
    vp = C.c_void_p
    if not device:
        f = lib.rs_host_road_votes_area_sweep
        f.argtypes = [vp] * 5 + [C.c_int] * 4 + [vp, C.c_int] + [vp] * 3
        _check(lib, f(*[a.ctypes.data for a in tabs], n, num_classes, slots, cap, thr.ctypes.data, T, *[a.ctypes.data for a in outs]), entry)
        return tuple(outs)
    import torch
    dev = [torch.from_numpy(a).cuda() for a in tabs + outs]
    torch.cuda.synchronize()
    f = lib.rs_op_road_votes_area_sweep
    f.argtypes = [vp] * 5 + [C.c_int] * 4 + [vp, C.c_int] + [vp] * 4
    _check(lib, f(*[a.data_ptr() for a in dev[:5]], n, num_classes, slots, cap, thr.ctypes.data, T, *[a.data_ptr() for a in dev[5:]], None), entry)
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in dev[5:])


def road_votes_area_sweep_host(b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float = 0.0):
    """``rs_host_road_votes_area_sweep`` on a dict with det_scores / det_classes (n, slots), det_count (n,), tile_first (n + 1,) and frac
    (n, slots, gt_cap) float64 -> wscore, wfrac (n, T, gt_cap, K) float64, pairs (n, T, gt_cap, K) int32.  Needs no device."""
    return _area_sweep_call("rs_host_road_votes_area_sweep", b, num_classes, thresholds, prefill, False)


def road_votes_area_sweep_device(b: Dict[str, np.ndarray], num_classes: int, thresholds, prefill: float = 0.0):
    """``rs_op_road_votes_area_sweep`` on the same dict, uploaded through torch: ``road_vote_area_sweep_kernel``'s tables."""
    return _area_sweep_call("rs_op_road_votes_area_sweep", b, num_classes, thresholds, prefill, True)


def vote_tables_polygons_host(polygons: Sequence, labels: Sequence[Sequence[Sequence[np.ndarray]]], scores: Sequence[np.ndarray],
                              classes: Sequence[np.ndarray], thresholds, num_classes: int = len(CLASS_NAMES)):
    """The host route to the tables ``Engine.road_votes_sweep(..., geometry="polygons")`` gives, through the host restatements (the
    device route's bits): polygons[tile] = ``engine.PolygonTables`` WITHOUT a flagged instance, or the nested polygon lists of
    ``vectorize.vectorize_masks_native`` (which fills in what the device flagged); labels[tile][label] = list of rings; scores[tile],
    classes[tile] (D_t,).  Returns per tile ``(wscore (T, L_t, K), wfrac (T, L_t, K), pairs (T, L_t, K), label_area (L_t,) float64)``.
    The fallback of a batch with a flagged instance and of one that does not fit the device pool: a tile's labels are taken 128 at a
    time, so nothing is truncated."""
    from .engine import PolygonTables
    thr = sweep_thresholds(thresholds)
    if not (len(polygons) == len(labels) == len(scores) == len(classes)):
        raise ValueError(f"{len(polygons)} polygon tables, {len(labels)} label lists, {len(scores)} score and {len(classes)} class arrays")
    out = []
    for tabs, labs, sc, cl in zip(polygons, labels, scores, classes):
        if not isinstance(tabs, PolygonTables):
            tabs = polygon_tables_from_lists(tabs)
        if len(tabs.flagged):
            raise ValueError("the host vote needs every instance's polygons: vectorise the flagged ones first (vectorize.vectorize_masks_native)")
        D = int(tabs.header.shape[0])
        if len(sc) != D or len(cl) != D:
            raise ValueError(f"{D} instances, {len(sc)} scores, {len(cl)} classes")
        det = stack_polygon_tables([tabs])
        slots = det["header"].shape[1]
        s_pad, c_pad = np.zeros((1, slots), np.float32), np.zeros((1, slots), np.int32)
        s_pad[0, :D], c_pad[0, :D] = np.asarray(sc, np.float32), np.asarray(cl, np.int32)
        parts = []
        for lo in range(0, max(len(labs), 1), 128):
            part = list(labs[lo:lo + 128])
            cap = max(len(part), 1)
            pool = pack_label_pool([part])
            frac, area, _ = polygon_overlaps_host({**det, **pool}, gt_cap=cap)
            ws, wa, pr = road_votes_area_sweep_host({"det_scores": s_pad, "det_classes": c_pad, "det_count": det["det_count"],
                                                     "tile_first": pool["tile_first"], "frac": frac}, num_classes, thr)
            parts.append((ws[0, :, :len(part)], wa[0, :, :len(part)], pr[0, :, :len(part)], area[0, :len(part)]))
        out.append((np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1),
                    np.concatenate([p[2] for p in parts], axis=1), np.concatenate([p[3] for p in parts])))
    return out
