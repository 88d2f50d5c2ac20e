"""The band histograms on the device (csrc/band_hist.h, band_hist_kernel in csrc/band_hist.hip): the operator against the host
restatement, ``Engine.band_hist`` against the numpy route on the same tiles and labels, behind every fetch form and beside the road
votes and the validation counts that share its pool, the ordering of the tile buffer against the next upload, the fallback of a batch
that does not fit, the streamed form of ``LanePipeline.run`` in both lane forms, and ``make_detections --road-stats``."""
import json
import os

import numpy as np
import pytest

from proj_roadsurf_amd import band_stats as B
from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd.engine import Engine, LanePipeline
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.synthetic import synthetic_tiles
from proj_roadsurf_amd.weights import synthetic_weights
from tests import band_hist_cases as V

pytestmark = pytest.mark.gpu
SPEC = dict(num_classes=2, min_size_test=192, max_size_test=320, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200)
THRESHOLD = 0.05


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("name", V.GPU_NAMES)
def test_operator_equals_host_restatement(gpu_required, name):
    b = V.case(name)
    want = B.band_hist_library_host(b["tiles"], b["packed"], b["tile_first"])
    first = B.band_hist_device(b["tiles"], b["packed"], b["tile_first"], prefill=0xFFFFFFF9)
    second = B.band_hist_device(b["tiles"], b["packed"], b["tile_first"], prefill=3)      # whatever the buffer held: the operator clears it
    assert first.dtype == np.uint32 and np.array_equal(first, want), int((first != want).sum())
    assert np.array_equal(second, want)
    assert want.sum() > 0
    if name == "side1024_c4":
        nodata = int((~b["tiles"][0].any(axis=2)).sum())
        assert nodata > 0 and first[0].sum(axis=1).tolist() == [2 ** 20 - nodata] * 4
    if name == "shapes_c3":                                                               # uniform tile, full-tile label: one bin per band
        assert first[5, 0, 7] == first[5, 1, 0] == first[5, 2, 200] == 72 * 72


def test_operator_without_instances_and_its_alignment_check(gpu_required):
    b = V.case("side32_c3")
    none = B.band_hist_device(b["tiles"], b["packed"][:0], np.zeros(4, np.int32))
    assert none.shape == (0, 3, 256)
    import torch
    from proj_roadsurf_amd.engine import load_library
    lib = load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc = lib.rs_op_band_hist(buf.data_ptr(), buf.data_ptr() + 1, buf.data_ptr(), 1, 1, 32, 3, buf.data_ptr(), None)
    assert rc == -1 and "aligned" in lib.rs_last_error().decode()


# ------------------------------------------------------------------------------------------------ engine
def _rect(x0, y0, x1, y1):
    return np.array([x0, y0, x1, y0, x1, y1, x0, y1], np.float64)


def _labels():
    """Per tile: a band across the tile, a label of two rings, a label that reaches the last column and row; tile 1 has a fourth."""
    base = [[_rect(0.0, 40.5, 128.0, 80.25)], [_rect(5.0, 5.0, 40.0, 60.0), _rect(70.5, 64.0, 120.0, 127.0)], [_rect(100.0, 90.0, 128.0, 128.0)]]
    return [base, base[::-1] + [[_rect(0.0, 0.0, 128.0, 128.0)]]]


@pytest.fixture(scope="module")
def small(gpu_required):
    spec = EngineSpec(**SPEC)
    W = synthetic_weights(spec, 0)
    tiles = np.array(synthetic_tiles(2, 128, 128, 3, seed=5))
    tiles[0, 50:60, 20:40] = 0                                      # nodata under the band across tile 0
    eng = Engine(spec, W, (128, 128, 3), max_batch=2)
    dets = eng.infer(tiles)
    labels = _labels()
    want = B.band_hist_host(tiles, labels)                          # the yardstick, once
    print(f"engine fixture: {[len(r) for r in dets]} detections, pixels per label {[w[:, 0].sum(axis=1).tolist() for w in want]}")
    assert all(int(w.sum()) > 0 for w in want) and int(want[0][0, 0].sum()) < 128 * 40
    yield spec, W, tiles, eng, dets, labels, want
    eng.close()


def _same(got, want):
    assert got is not None and len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == np.uint32 and np.array_equal(g, w), int((g != w).sum())


def _same_dets(res, dets, masks=True):
    for r, d in zip(res, dets):
        assert np.array_equal(r.scores.view(np.uint32), d.scores.view(np.uint32)) and np.array_equal(r.pred_classes, d.pred_classes)
        assert np.array_equal(r.pred_boxes.view(np.uint32), d.pred_boxes.view(np.uint32))
        if masks:
            assert np.array_equal(r.pred_masks, d.pred_masks)


def test_engine_histograms_equal_the_numpy_route(small):
    spec, W, tiles, eng, dets, labels, want = small
    _same(eng.band_hist(tiles, labels), want)
    _same(eng.band_hist(tiles, labels), want)                       # the pool and the table are reused
    assert eng.band_fallbacks == 0 and eng.eval_fallbacks == 0 and eng.vote_fallbacks == 0
    _same(eng.band_hist(tiles[1:], labels[1:]), want[1:])           # a ragged batch of one tile
    _same(eng.band_hist(tiles, [[], labels[1]]), [np.zeros((0, 3, 256), np.uint32), want[1]])
    _same(eng.band_hist(tiles, [[], []]), [np.zeros((0, 3, 256), np.uint32)] * 2)      # no label at all: nothing to count or copy


@pytest.mark.parametrize("form", ["crops", "polygons", "canvas"])
def test_histograms_follow_a_fetch_and_the_votes_of_the_same_forward(small, form):
    spec, W, tiles, eng, dets, labels, want = small
    votes = RV.vote_tables_host(dets, labels, 2, THRESHOLD)
    for hist_first in (False, True):                                # both orders of the waits
        eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)
        eng.fetch_async(2, crops=form == "crops", polygons=form == "polygons")
        assert eng.road_votes(2, labels, THRESHOLD, wait=False) is True
        assert eng.band_hist(2, labels, wait=False) is True
        if hist_first:
            _same(eng.band_hist_wait(2), want)
            got_votes = eng.road_votes_wait(2)
            res = eng.fetch_wait(2)
        else:
            res = eng.fetch_wait(2)
            got_votes = eng.road_votes_wait(2)
            _same(eng.band_hist_wait(2), want)
        _same_dets(res, dets, masks=form != "polygons")
        _same_dets([g[0] for g in got_votes], dets, masks=False)
        for g, w in zip(got_votes, votes):                          # bit-identical to a run without the histograms
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g[1:], w))
    # and in front of the votes
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 2)
    assert eng.band_hist(2, labels, wait=False) is True
    got_votes = eng.road_votes(2, labels, THRESHOLD)
    _same(eng.band_hist_wait(2), want)
    for g, w in zip(got_votes, votes):
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g[1:], w))


def test_validation_counts_share_the_pool_and_keep_their_results(small):
    spec, W, tiles, eng, dets, labels, want = small
    gts = [[[_rect(10.0, 10.0, 70.0, 50.0)], [_rect(64.0, 64.0, 128.0, 128.0)]], [[_rect(0.0, 0.0, 128.0, 128.0)]]]
    before = eng.eval_counts(tiles, gts)
    _same(eng.band_hist(tiles, labels), want)
    after = eng.eval_counts(tiles, gts)
    for b, a in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(b[1:], a[1:]))
    assert after[1][3].tolist() == [128 * 128] and after[0][3].tolist() == [60 * 40, 64 * 64]
    _same(eng.band_hist(tiles, labels), want)


@pytest.mark.parametrize("route", ["upload_async", "infer", "staging_copy", "upload_tiles"])
def test_the_next_upload_waits_for_the_histogram_kernel(small, route):
    """Every way of writing the engine's tile buffer while a band-histogram fetch is outstanding: the histograms are those of the
    batch they were asked for, the next forward's detections those of a clean run.  The values decide, not the timing: a kernel
    that read the second batch's tiles would count other pixels."""
    spec, W, tiles, eng, dets, labels, want = small
    other = np.ascontiguousarray(255 - tiles[::-1])
    clean = eng.infer(other)
    assert not np.array_equal(np.concatenate(B.band_hist_host(other, labels)), np.concatenate(want))
    assert eng.band_hist(tiles, labels, wait=False) is True
    if route == "upload_async":
        eng.infer_device(eng.upload_async(other), 2)
        eng.fetch_async(2, crops=False)
        second = None
    elif route == "infer":
        second = eng.infer(other)
    elif route == "staging_copy":
        import torch
        elsewhere = torch.from_numpy(other).cuda()
        torch.cuda.synchronize()
        eng.infer_device(elsewhere.data_ptr(), 2)
        eng.fetch_async(2, crops=False)
        second = None
    else:
        eng.infer_device(eng.upload_tiles(other), 2)
        eng.fetch_async(2, crops=False)
        second = None
    got = eng.band_hist_wait(2)
    if second is None:
        second = eng.fetch_wait(2)
    _same(got, want)
    _same_dets(second, clean)
    _same(eng.band_hist(tiles, labels), want)
    _same_dets(eng.infer(tiles), dets)


# ------------------------------------------------------------------------------------------------ fallback and the streamed form
def _many(labels):
    return [labels[0], [[_rect(10.0 + (i % 7), 10.0, 60.0, 70.0)] for i in range(129)]]


def test_a_tile_with_129_labels_does_not_fit(small):
    spec, W, tiles, eng, dets, labels, want = small
    eng.band_fallbacks = 0
    eng.sync()
    assert eng.band_hist(2, _many(labels)) is None and eng.band_fallbacks == 1 and eng.eval_fallbacks == 0 and eng.vote_fallbacks == 0
    assert eng._band_pending is False                               # nothing was enqueued
    _same(eng.band_hist(tiles, labels), want)                       # the next fitting batch
    eng.band_fallbacks = 0
    with pytest.raises(ValueError):
        eng.band_hist(tiles, labels[:1])


def _batches(tiles):
    return [tiles, tiles[::-1].copy(), tiles]


@pytest.fixture(scope="module", params=[False, True], ids=["independent_lanes", "shared_stream"])
def pipe(request, small):
    spec, W, tiles, eng, dets, labels, want = small
    p = LanePipeline(spec, W, (128, 128, 3), max_batch=2, lanes=2, shared_stream=request.param)
    yield p
    p.close()


def _bits(res):
    return [(r.pred_boxes.tobytes(), r.scores.tobytes(), r.pred_classes.tobytes(), r.pred_masks.tobytes()) for r in res]


def test_pipeline_with_band_stats_equals_the_host_route(small, pipe):
    spec, W, tiles, eng, dets, labels, want = small
    batches = _batches(tiles)
    many = _many(labels)
    labs = [labels, many, labels]                                   # one batch of the stream does not fit
    wants = [B.band_hist_host(b, l) for b, l in zip(batches, labs)]
    plain = [_bits(res) for res in pipe.run(iter(batches))]
    assert all(not hasattr(r, "band_hist") and not hasattr(r, "road_votes") for res in pipe.run(iter(batches)) for r in res)
    # histograms alone
    got = list(pipe.run(iter(batches), labels=iter(labs), band_stats=True, road_votes=False))
    assert len(got) == 3 and pipe.band_fallbacks == 1
    for res, w, p in zip(got, wants, plain):
        _same([r.band_hist for r in res], w)
        assert _bits(res) == p and all(not hasattr(r, "road_votes") for r in res)
    assert got[1][1].band_hist.shape == (129, 3, 256)
    # with the votes
    votes = [[row[1:] for row in eng.road_votes(b, l, THRESHOLD)] for b, l in ((batches[0], labels), (batches[2], labels))]
    got = list(pipe.run(iter(batches), labels=iter(labs), vote_threshold=THRESHOLD, band_stats=True))
    assert pipe.band_fallbacks == 1 and pipe.vote_fallbacks == 1
    for res, w, p in zip(got, wants, plain):
        _same([r.band_hist for r in res], w)
        assert _bits(res) == p
    for res, v in ((got[0], votes[0]), (got[2], votes[1])):
        for r, w in zip(res, v):
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(r.road_votes, w))
    # labels with the switch off: votes as before, no histograms
    again = list(pipe.run(iter(batches), labels=iter([labels] * 3), vote_threshold=THRESHOLD))
    assert all(hasattr(r, "road_votes") and not hasattr(r, "band_hist") for res in again for r in res)
    assert [_bits(res) for res in again] == plain
    with pytest.raises(ValueError):
        list(pipe.run(iter(batches), band_stats=True))


# ------------------------------------------------------------------------------------------------ the CLI
N_TILES, TILE, BATCH = 6, 128, 4


def _ring(x0, y0, x1, y1):
    return [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]


def _dataset(tmp_path):
    """The working directory of tests/test_gpu_road_votes_cli.py: road "A" crosses tiles 0..2 (category 1), "B" tiles 2..4 (category
    2), every tile has a road of its own, tile 5 a label of two rings."""
    import yaml
    from PIL import Image
    from tests.util import synthetic_tiles as util_tiles
    wd = tmp_path / "outputs" / "obj_detector"
    (wd / "val-images").mkdir(parents=True)
    tiles = np.array(util_tiles(N_TILES, TILE, TILE, 3, seed=9))
    tiles[1, 30:50, 10:90] = 0                                      # nodata under road "A"
    images, anns = [], []

    def ann(image, seg, cat=1, **kw):
        anns.append(dict({"id": 100 + len(anns), "image_id": image, "category_id": cat, "segmentation": seg, "iscrowd": 0}, **kw))
    for i in range(N_TILES):
        fn = f"val-images/18_{100 + i}_200.tif"
        Image.fromarray(tiles[i][:, :, ::-1]).save(str(wd / fn))
        images.append({"id": i, "file_name": fn, "width": TILE, "height": TILE})
        if i <= 2:
            ann(i, [_ring(0, 20, 128, 70)], road_id="A")
        if 2 <= i <= 4:
            ann(i, [_ring(40.5, 0, 100, 128)], cat=2, road_id="B")
        ann(i, [_ring(10, 60, 120, 125.5)], cat=1 + i % 2)
    ann(5, [_ring(0, 0, 60, 60), _ring(64, 64, 128, 128)], road_id="two_rings")
    ann(1, [_ring(0, 0, 128, 128)], road_id="crowd", iscrowd=1)
    cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
    json.dump({"images": images, "annotations": anns, "categories": cats}, open(wd / "COCO_val.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200}, "ROI_HEADS": {"NUM_CLASSES": 1}},
          "TEST": {"DETECTIONS_PER_IMAGE": 20}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"make_detections.py": {"working_directory": str(wd), "log_subfolder": "logs", "COCO_files": {"val": "COCO_val.json"},
                                  "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {"pth_file": "logs/model_0005999.pth"},
                                  "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return str(tmp_path / "config.yaml"), wd, images, anns


def test_road_stats_switch_writes_the_host_table(gpu_required, tmp_path):
    from proj_roadsurf_amd import make_detections
    from proj_roadsurf_amd.decode_pool import read_tile
    cfg, wd, images, anns = _dataset(tmp_path)
    tiles = np.stack([read_tile(str(wd / e["file_name"])) for e in images])
    mine = [[a for a in anns if a["image_id"] == e["id"] and not a["iscrowd"]] for e in images]
    labels = [[[np.array(r) for r in a["segmentation"]] for a in row] for row in mine]
    ids = [[a.get("road_id", a["id"]) for a in row] for row in mine]
    by_road = B.reduce_band_hist(B.band_hist_host(tiles, labels), ids)
    cover = {}
    for row in mine:
        for a in row:
            cover.setdefault(a.get("road_id", a["id"]), {1: "artificial", 2: "natural"}[a["category_id"]])
    want = {"columns": list(B.COLUMNS), "roads": [{"road_id": rid, "bands": B.json_rows(B.stats_from_hist(h))} for rid, h in by_road.items()],
            "covers": [{"cover_type": c, "bands": B.json_rows(rows)} for c, rows in B.cover_stats(by_road, cover).items()]}
    cwd = os.getcwd()
    try:
        assert make_detections.main([cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0", "--road-stats"]) == 0
    finally:
        os.chdir(cwd)
    got = json.load(open(wd / "val_road_stats.json"))
    assert got == json.loads(json.dumps(want))
    assert [r["road_id"] for r in got["roads"]] == ["A", 101, 103, "B", 106, 108, 110, 111, "two_rings"]
    assert [c["cover_type"] for c in got["covers"]] == ["artificial", "natural"] and not (wd / "val_road_votes.json").exists()
    a = got["roads"][0]["bands"]
    assert len(a) == 3 and 0 < a[0]["count"] <= 3 * 128 * 50 - 20 * 80 and a[0]["min"] is not None
