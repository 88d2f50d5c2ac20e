"""The device polygoniser (csrc/polygonize.hip) against the host vectoriser (csrc/vectorize.cpp) on the same bytes, array for array:
the stand-alone operator, the host fallback of instances beyond the kernel's capacities, the engine's polygon fetch, the lane
pipeline and the CLI."""
import ctypes as C
import json
import logging
import os
import sqlite3

import numpy as np
import pytest

from oracle import host_tail_oracle as O
from proj_roadsurf_amd import vectorize as V
from proj_roadsurf_amd.engine import Engine, Predictor, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests import polygonize_ref as R
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu

CANVASES = ((11, 13), (24, 40))            # (h, w): a width that is no multiple of 8, and several bytes per row
STAIR_EPS = 0.7071067811865476


def _vec_arrays(lib, r):
    c = [C.c_int64() for _ in range(4)]
    lib.rs_vec_counts(r, *[C.byref(x) for x in c])
    ni, npoly, nr, nv = (int(x.value) for x in c)
    ipc = np.zeros(ni, np.int32); prc = np.zeros(npoly, np.int32); rl = np.zeros(nr, np.int32); xy = np.zeros((nv, 2), np.float64)
    assert lib.rs_vec_copy(r, ipc.ctypes.data_as(C.POINTER(C.c_int32)), prc.ctypes.data_as(C.POINTER(C.c_int32)),
                           rl.ctypes.data_as(C.POINTER(C.c_int32)), xy.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return ipc, prc, rl, xy


def _host_arrays(packed, h, w, eps):
    lib = load_library()
    r = lib.rs_vectorize_masks(packed.ctypes.data_as(C.c_void_p), packed.shape[0], h, w, float(eps), 1)
    assert r
    try:
        return _vec_arrays(lib, r)
    finally:
        lib.rs_vec_free(r)


def _device_arrays(tables, packed, h, w):
    """The four arrays of the device tables, the flagged instances merged in from the host (rs_vec_from_tables)."""
    lib = load_library()
    wb = (w + 7) // 8
    n = packed.shape[0]
    rects = np.tile(np.array([0, 0, wb, h], np.int32), (n, 1))
    offs = (np.arange(n, dtype=np.int64) * h * wb).astype(np.uint32)
    r = V._result_from_polygons(lib, tables, (rects, offs, packed.reshape(-1)), h, w, tables.rdp_epsilon, 1)
    try:
        return _vec_arrays(lib, r)
    finally:
        lib.rs_vec_free(r)


def _assert_same(got, want, what):
    for name, a, b in zip(("inst_poly_count", "poly_ring_count", "ring_len", "xy"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f"{what}: {name} differs"


def _oracle_lists(masks, eps):
    out = []
    for m in masks:
        polys = []
        for poly in O.mask_to_polygons(m):
            rings = []
            for r in poly:
                rr = O.rdp(r, eps) if eps > 0 else list(r)
                rings.append([tuple(p) for p in (rr if len(rr) >= 4 else r)])
            polys.append(rings)
        out.append(polys)
    return out


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("eps", [0.0, 0.75])
@pytest.mark.parametrize("hw", CANVASES, ids=["13x11", "40x24"])
def test_structured_masks_equal_host_and_oracle(gpu_required, hw, eps):
    h, w = hw
    named = R.structured_masks(h, w)
    masks = np.stack(list(named.values()))
    packed = R.pack(masks)
    t = V.polygonize_masks_device(packed, h, w, eps)
    assert not len(t.flagged), f"flagged with the default caps: {[list(named)[i] for i in t.flagged]}"
    _assert_same(_device_arrays(t, packed, h, w), _host_arrays(packed, h, w, eps), f"{w}x{h} eps {eps}")
    assert V.polygon_tables_to_lists(t, packed, h, w) == _oracle_lists(masks, eps)


@pytest.mark.parametrize("eps", [0.0, 0.75])
@pytest.mark.parametrize("hw", CANVASES, ids=["13x11", "40x24"])
def test_random_masks_equal_host(gpu_required, hw, eps):
    h, w = hw
    for dens in (0.2, 0.5, 0.8):
        for seed in range(3):
            packed = R.pack(R.random_masks(32, h, w, dens, 1000 * seed + int(dens * 10)))
            t = V.polygonize_masks_device(packed, h, w, eps)
            assert not len(t.flagged)
            _assert_same(_device_arrays(t, packed, h, w), _host_arrays(packed, h, w, eps), f"{w}x{h} density {dens} seed {seed} eps {eps}")


@pytest.mark.parametrize("hw", CANVASES, ids=["13x11", "40x24"])
def test_staircases_at_the_corner_distance(gpu_required, hw):
    """epsilon = 1 / sqrt(2) as a double: the distance of a unit stair corner from its diagonal chord, so the rounded fp64 quotient decides."""
    h, w = hw
    masks = np.stack(list(R.staircase_masks(h, w).values()))
    packed = R.pack(masks)
    for eps in (STAIR_EPS, np.nextafter(STAIR_EPS, 0.0), np.nextafter(STAIR_EPS, 1.0)):
        t = V.polygonize_masks_device(packed, h, w, float(eps))
        assert not len(t.flagged)
        _assert_same(_device_arrays(t, packed, h, w), _host_arrays(packed, h, w, float(eps)), f"staircases {w}x{h} eps {eps!r}")
    assert V.polygon_tables_to_lists(V.polygonize_masks_device(packed, h, w, STAIR_EPS), packed, h, w) == _oracle_lists(masks, STAIR_EPS)


def test_operator_is_deterministic_and_handles_one_instance(gpu_required):
    h, w = 24, 40
    packed = R.pack(R.random_masks(32, h, w, 0.5, 7))
    a = V.polygonize_masks_device(packed, h, w, 0.75)
    b = V.polygonize_masks_device(packed, h, w, 0.75)
    for x, y in ((a.header, b.header), (a.poly_ring_count, b.poly_ring_count), (a.ring_len, b.ring_len), (a.xy, b.xy)):
        assert np.array_equal(x, y)
    one = V.polygonize_masks_device(packed[5:6], h, w, 0.75)
    _assert_same(_device_arrays(one, packed[5:6], h, w), _host_arrays(packed[5:6], h, w, 0.75), "one instance")


# ------------------------------------------------------------------------------------------------ fallback
@pytest.mark.parametrize("caps", [dict(edge_cap=16), dict(vertex_cap=8)], ids=["edge_cap_16", "vertex_cap_8"])
def test_instances_over_a_cap_are_flagged_and_merged_from_the_host(gpu_required, caps):
    h, w = 24, 40
    named = R.structured_masks(h, w)
    big = {"checkerboard8": named["checkerboard8"], "random": R.random_masks(1, h, w, 0.5, 3)[0]}
    small = {k: named[k] for k in ("empty", "pixel_first", "pixel_last")}           # 4 edges, 5 vertices: under both caps
    order = ["empty", "checkerboard8", "pixel_first", "random", "pixel_last"]
    masks = np.stack([{**big, **small}[k] for k in order])
    packed = R.pack(masks)
    for eps in (0.0, 0.75):
        t = V.polygonize_masks_device(packed, h, w, eps, **caps)
        assert t.flagged.tolist() == [1, 3], f"flags {t.header[:, 0].tolist()}"
        assert not t.header[[1, 3], 1:4].any()                                      # a flagged instance has no rows of its own
        _assert_same(_device_arrays(t, packed, h, w), _host_arrays(packed, h, w, eps), f"merged, {caps}, eps {eps}")


# ------------------------------------------------------------------------------------------------ engine
SMALL = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)


@pytest.fixture(scope="module")
def small(gpu_required):
    spec = EngineSpec(**SMALL)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 128, 128, 3, seed=77)
    eng = Engine(spec, W, (128, 128, 3), max_batch=3)
    yield spec, W, tiles, eng
    eng.close()


def _run(eng, tiles, **fetch):
    n = tiles.shape[0]
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), n)
    eng.fetch_async(n, **fetch)
    return eng.fetch_wait(n)


def _lists(inst, eps):
    h, w = inst.image_size
    if getattr(inst, "_polygons", None) is not None:
        return V.vectorize_masks_native(None, h, w, eps, 1, polygons=inst._polygons, crops=inst._crops)
    return V.vectorize_masks_native(inst._packed, h, w, eps, 1) if len(inst) else []


def _same_dets(a, b):
    return (np.array_equal(a.pred_boxes.view(np.uint32), b.pred_boxes.view(np.uint32)) and np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32))
            and np.array_equal(a.pred_classes, b.pred_classes))


@pytest.mark.parametrize("n", [3, 2], ids=["full_batch", "ragged_batch"])
def test_engine_polygons_equal_crops_plus_host_vectoriser(small, n):
    spec, W, tiles, eng = small
    ref = _run(eng, tiles[:n], crops=True)
    assert sum(len(r) for r in ref) > 0
    traced = flagged = 0
    for eps in (0.75, 0.0):
        got = _run(eng, tiles[:n], polygons=True, rdp_epsilon=eps)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert _same_dets(g, r), f"tile {i}: detections differ"
            assert g._polygons is not None and g._polygons.rdp_epsilon == eps
            assert g.has("pred_masks") == (g._crops is not None)
            assert _lists(g, eps) == _lists(r, eps), f"tile {i} eps {eps}: polygons differ"
            rows_g = V.instances_to_gpkg_rows(g, f"t{i}.tif", (0.0, 0.0, 64.0, 64.0), eps > 0, eps, srs_id=3857)
            assert rows_g == V.instances_to_gpkg_rows(r, f"t{i}.tif", (0.0, 0.0, 64.0, 64.0), eps > 0, eps, srs_id=3857)
            flagged += len(g._polygons.flagged)
            traced += len(g) - len(g._polygons.flagged)
    print(f"engine polygons: {traced} instances traced on the device, {flagged} left to the host ({flagged / max(traced + flagged, 1):.1%})")
    assert traced > 0
    # masks on request: the same polygons, and the crops come along
    with_masks = _run(eng, tiles[:n], polygons=True, rdp_epsilon=0.75, masks=True)
    for g, r in zip(with_masks, ref):
        assert g.has("pred_masks") and np.array_equal(g._packed, r._packed)


FETCH_ORDER = ("canvas", "canvas", "crops", "crops", "polygons", "polygons", "canvas", "polygons+masks", "crops", "canvas", "polygons", "crops")
FETCH_ARGS = {"canvas": dict(crops=False), "crops": dict(crops=True), "polygons": dict(polygons=True, rdp_epsilon=0.75),
              "polygons+masks": dict(polygons=True, rdp_epsilon=0.75, masks=True)}


def test_fetch_kinds_in_every_order(small):
    """One engine, a forward on the same tiles before every fetch, the three kinds of fetch in an order that holds every ordered pair of
    distinct kinds and each kind twice in a row: whatever was fetched before, a fetch gives the synchronous fetch's detections, the
    canvas and crops fetches its mask bits, the polygon fetch the polygons of the crops."""
    spec, W, tiles, eng = small
    kinds = [k.split("+")[0] for k in FETCH_ORDER]
    pairs = set(zip(kinds, kinds[1:]))
    assert pairs >= {(a, b) for a in ("canvas", "crops", "polygons") for b in ("canvas", "crops", "polygons")}
    for n in (3, 2):
        crops_lists = [_lists(r, 0.75) for r in _run(eng, tiles[:n], crops=True)]
        for step, what in enumerate(FETCH_ORDER):
            got = _run(eng, tiles[:n], **FETCH_ARGS[what])
            ref = eng.fetch(n)                                    # the same forward, copied on the forward's own stream
            assert len(got) == len(ref) == n and sum(len(r) for r in ref) > 0
            flagged = any(len(g._polygons.flagged) for g in got) if what.startswith("polygons") else False
            for i, (g, r) in enumerate(zip(got, ref)):
                where = f"n {n} step {step} ({what}) tile {i}"
                assert _same_dets(g, r), f"{where}: detections differ"
                if what.startswith("polygons"):
                    assert g._polygons is not None and g._polygons.rdp_epsilon == 0.75, where
                    assert _lists(g, 0.75) == crops_lists[i], f"{where}: polygons differ"
                    assert g.has("pred_masks") == (what == "polygons+masks" or flagged), where
                    if g.has("pred_masks"):
                        assert np.array_equal(g.pred_masks, r.pred_masks), f"{where}: mask bits differ"
                else:
                    assert g._polygons is None and (g._crops is not None) == (what == "crops"), where
                    assert g.pred_masks.dtype == r.pred_masks.dtype and np.array_equal(g.pred_masks, r.pred_masks), f"{where}: mask bits differ"
                    assert _lists(g, 0.75) == crops_lists[i], f"{where}: polygons differ"


def _crop_edge_counts(inst):
    """E of every instance of a tile from its crop bytes, the crop taken as a mask of its own (what the kernel counts)."""
    rects, offs, data = inst._crops
    w = inst.image_size[1]
    out = []
    for (x0b, oy, wb, rows), o in zip(np.asarray(rects).tolist(), np.asarray(offs).tolist()):
        bits = np.unpackbits(np.asarray(data[o:o + wb * rows], np.uint8).reshape(rows, wb), axis=1, bitorder="little").astype(bool)
        out.append(R.edge_count(bits[:, :min(8 * wb, w - 8 * x0b)]))
    return out


def test_engine_fallback_forced_by_the_edge_cap_switch(small, monkeypatch):
    """RS_POLY_EDGE_CAP at the median edge count of the batch's own crops: about half of the instances are left to the host, their
    crops come along, and polygons and GeoPackage rows are those of crops + host vectoriser.  Without the switch, no crop travels
    unless an instance is over the kernel's real capacities."""
    spec, W, tiles, eng = small
    ref = _run(eng, tiles, crops=True)
    counts = [_crop_edge_counts(r) for r in ref]
    flat = np.array([e for c in counts for e in c])
    cap = int(np.median(flat))
    assert len(flat) > 1 and cap >= 1 and flat.max() > cap, f"the edge counts of the crops do not straddle their median: {sorted(flat.tolist())}"

    def check(e2, eps, want_flags):
        got = _run(e2, tiles, polygons=True, rdp_epsilon=eps)
        traced = flagged = 0
        any_flagged = any(len(g._polygons.flagged) for g in got)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert _same_dets(g, r), f"tile {i}: detections differ"
            flags = g._polygons.header[:, 0] != 0
            ec = np.array(counts[i])
            if want_flags:
                assert flags[ec > cap].all(), f"tile {i}: an instance over the cap was traced"
                assert not flags[ec <= min(cap, 2048)].any(), f"tile {i}: an instance under every cap was flagged"     # R <= E / 4, V <= E + R
            assert (g._crops is not None) == any_flagged                     # the batch's crops travel exactly when one of its instances needs them
            assert not g._polygons.header[flags, 1:4].any()
            assert _lists(g, eps) == _lists(r, eps), f"tile {i} eps {eps}: polygons differ"
            rows_g = V.instances_to_gpkg_rows(g, f"t{i}.tif", (0.0, 0.0, 64.0, 64.0), eps > 0, eps, srs_id=3857)
            assert rows_g == V.instances_to_gpkg_rows(r, f"t{i}.tif", (0.0, 0.0, 64.0, 64.0), eps > 0, eps, srs_id=3857)
            flagged += int(flags.sum())
            traced += len(g) - int(flags.sum())
        return traced, flagged, got

    try:
        with monkeypatch.context() as mp:
            mp.setenv("RS_POLY_EDGE_CAP", str(cap))
            e2 = Engine(spec, W, (128, 128, 3), max_batch=3)                 # the switches are read when an engine is created
            try:
                for eps in (0.0, 0.75):
                    traced, flagged, got = check(e2, eps, True)
                    print(f"engine fallback, edge cap {cap} (median of {len(flat)} crops, E {int(flat.min())}..{int(flat.max())}), eps {eps}: {traced} traced, {flagged} left to the host")
                    assert flagged > 0 and traced > 0
                    assert flagged >= int((flat > cap).sum())
                    assert all(g._crops is not None for g in got if len(g))
            finally:
                e2.close()
    finally:
        monkeypatch.delenv("RS_POLY_EDGE_CAP", raising=False)
        e3 = Engine(spec, W, (128, 128, 3), max_batch=3)                     # reads the switches again: the kernel's own caps
    try:
        traced, flagged, got = check(e3, 0.75, False)
        assert traced > 0
        if flagged:
            print(f"engine fallback: {flagged} instance(s) are over the kernel's capacities without the switch; the no-crops assertion is not made")
        else:
            assert all(g._crops is None for g in got)
    finally:
        e3.close()


def test_forward_after_a_polygon_fetch_repeats_the_first(small):
    """The engine's result buffers are free once the polygon fetch says so: another forward gives the first one's bits."""
    spec, W, tiles, eng = small
    first = _run(eng, tiles, polygons=True, rdp_epsilon=0.75)
    lists = [_lists(g, 0.75) for g in first]
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 3)
    eng.fetch_async(3, polygons=True, rdp_epsilon=0.75)
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 3)        # enqueued while the polygon copy may still be in flight
    second = eng.fetch_wait(3)
    eng.fetch_async(3, crops=True)
    third = eng.fetch_wait(3)
    for a, b, c in zip(first, second, third):
        assert _same_dets(a, b) and _same_dets(a, c)
    assert [_lists(g, 0.75) for g in second] == lists
    assert [_lists(g, 0.75) for g in third] == lists


def test_one_tile_path_with_polygons(small):
    """n = 1 replays the captured graph of the forward; the polygon fetch runs behind it."""
    spec, W, tiles, eng = small
    for k in range(3):
        t = tiles[k:k + 1]
        ref = _run(eng, t, crops=True)[0]
        got = _run(eng, t, polygons=True, rdp_epsilon=0.75)[0]
        assert _same_dets(got, ref)
        assert _lists(got, 0.75) == _lists(ref, 0.75)


# ------------------------------------------------------------------------------------------------ pipeline
def test_predict_stream_device_rows_equal_host_rows(gpu_required):
    spec = EngineSpec(**SMALL)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(14, 128, 128, 3, seed=5)
    batches = [[tiles[i] for i in range(k, min(k + 3, 14))] for k in range(0, 14, 3)]     # 5 batches, the last one ragged
    assert len(batches) == 5
    rows = {}
    for mode in ("host", "device"):
        p = Predictor(spec, W, max_batch=3, lanes=2, on_saturation="ignore", vectorize=mode, rdp_epsilon=0.75)
        try:
            out = []
            for res in p.predict_stream(iter(batches)):
                for o in res:
                    inst = o["instances"]
                    assert (getattr(inst, "_polygons", None) is not None) == (mode == "device")
                    out.append(V.instances_to_gpkg_rows(inst, f"tile{len(out)}.tif", (10.0, 20.0, 74.0, 84.0), True, 0.75, srs_id=2056))
            rows[mode] = out
        finally:
            p.close()
    assert len(rows["host"]) == 14 and sum(len(r[0]) for r in rows["host"]) > 0
    assert rows["device"] == rows["host"]                        # blobs byte for byte, scores, classes, names, bbox


# ------------------------------------------------------------------------------------------------ CLI
def _cli_dataset(tmp_path, n_tiles, tile=128):
    from PIL import Image
    import yaml
    wd = tmp_path / "outputs" / "obj_detector"
    (wd / "val-images").mkdir(parents=True)
    tiles = synthetic_tiles(n_tiles, tile, tile, 3, seed=9)
    images, meta = [], {}
    for i in range(n_tiles):
        fn = f"val-images/18_{100 + i}_200.tif"
        Image.fromarray(tiles[i][:, :, ::-1]).save(str(wd / fn))
        images.append({"id": i, "file_name": fn, "width": tile, "height": tile})
        meta[fn] = {"extent": [1000.0 * i, 0.0, 1000.0 * i + 52.0, 52.0], "crs": "EPSG:3857"}
    cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
    json.dump({"images": images, "annotations": [], "categories": cats}, open(wd / "COCO_val.json", "w"))
    json.dump(meta, open(wd / "img_metadata.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200}, "ROI_HEADS": {"NUM_CLASSES": 1}},
          "TEST": {"DETECTIONS_PER_IMAGE": 20}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"make_detections.py": {"working_directory": str(wd), "log_subfolder": "logs", "image_metadata_json": "img_metadata.json", "COCO_files": {"val": "COCO_val.json"},
                                  "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {"pth_file": "logs/model_0005999.pth"},
                                  "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return str(tmp_path / "config.yaml"), wd


def test_cli_device_geopackage_equals_host_geopackage(gpu_required, tmp_path, caplog):
    from proj_roadsurf_amd import make_detections
    cfg, wd = _cli_dataset(tmp_path, 21)                        # batches of 4: five full ones and a ragged last one
    name = "val_detections_at_0dot05_threshold"
    common = [cfg, "--synthetic-weights", "--batch", "4", "--tagged-samples", "0", "--decode-procs", "0"]
    cwd = os.getcwd()
    try:
        assert make_detections.main(common) == 0
        os.chdir(cwd)
        os.rename(wd / f"{name}.gpkg", wd / "host.gpkg")
        with caplog.at_level(logging.INFO, logger="make_detections"):
            assert make_detections.main(common + ["--vectorize", "device"]) == 0
    finally:
        os.chdir(cwd)
    q = f'SELECT fid, geom, score, det_class, image FROM "{name}" ORDER BY fid'
    a, b = sqlite3.connect(str(wd / "host.gpkg")), sqlite3.connect(str(wd / f"{name}.gpkg"))
    try:
        ra, rb = a.execute(q).fetchall(), b.execute(q).fetchall()
        assert len(ra) > 21 and ra == rb, f"{len(ra)} rows against {len(rb)}"
        cq = "SELECT min_x, min_y, max_x, max_y, srs_id FROM gpkg_contents"
        assert a.execute(cq).fetchall() == b.execute(cq).fetchall()
    finally:
        a.close(); b.close()
    assert any("instances fell back to the host vectoriser" in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records][-5:]
