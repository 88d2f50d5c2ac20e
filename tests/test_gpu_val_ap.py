"""Validation AP on the device (csrc/val_ap.hip, ``Engine.eval_counts``, ``train_model --val-ap device``): the full-canvas rasteriser
against the host rasteriser bit for bit, the pair counts against numpy, the engine's counts against counts taken from ``infer()``'s
masks, the fallbacks, and the command line.  Every comparison is exact."""
import json
import logging
import os

import numpy as np
import pytest

from proj_roadsurf_amd import coco_eval
from proj_roadsurf_amd.engine import Engine
from proj_roadsurf_amd.raster_vote import pair_counts_device
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.train_targets import rasterize_canvases_device, rasterize_polygons_within_box
from proj_roadsurf_amd.weights import synthetic_weights
from tests.util import synthetic_tiles
from tests.val_ap_cases import FAMILIES, family, host_masks, unpack

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ rasteriser operator
@pytest.mark.parametrize("name", FAMILIES)
def test_canvas_rasteriser_equals_host_per_family(gpu_required, name):
    """Sides below, at and above one 32-column strip, with rows of whole words (64, 256) and of odd byte counts (8, 30, 250)."""
    for side in (8, 30, 64, 250, 256):
        n = 6 if side >= 250 else 24
        want = host_masks(name, side, n)
        got = unpack(rasterize_canvases_device(family(name, side, n), side, packed=True), side)
        assert np.array_equal(got, want), (name, side, int((got != want).sum()))
        if name not in ("full", "outside"):
            assert 0.01 < want.mean() < 0.99
    assert host_masks("full", 64, 24).all() and not host_masks("outside", 64, 24).any()


def test_canvas_rasteriser_at_side_1024(gpu_required):
    """One call, 8 instances (one per family): 32 strips per instance, 128-byte rows."""
    inst = [family(name, 1024, 1, seed=3)[0] for name in FAMILIES]
    want = np.stack([rasterize_polygons_within_box(p, np.array([0.0, 0.0, 1024.0, 1024.0]), 1024) for p in inst])
    got = unpack(rasterize_canvases_device(inst, 1024, packed=True), 1024)
    assert np.array_equal(got, want)
    assert 0.01 < want[:6].mean() < 0.99 and want[6].all() and not want[7].any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256])
def test_canvas_rasteriser_instance_counts(gpu_required, n):
    inst = family("inside", 64, 256)[:n]
    got = rasterize_canvases_device(inst, 64)
    assert got.shape == (n, 64, 64) and np.array_equal(got, host_masks("inside", 64, 256)[:n])


def test_canvas_rasteriser_instance_without_polygons(gpu_required):
    inst = family("hole", 64, 5)
    inst.insert(2, [])
    inst.append([])
    want = host_masks("hole", 64, 5)
    got = rasterize_canvases_device(inst, 64)
    assert not got[2].any() and not got[6].any()
    assert np.array_equal(got[[0, 1, 3, 4, 5]], want)


# ------------------------------------------------------------------------------------------------ pair counts
def _random_packed(rng, shape, side, density):
    bits = rng.random(shape + (side, side)) < density
    return np.packbits(bits, axis=-1, bitorder="little"), bits


@pytest.mark.parametrize("side", [30, 64, 250])
@pytest.mark.parametrize("counts,gts", [((100,), (7,)), ((1,), (128,)), ((0,), (1,)), ((100,), (0,)), ((0, 1, 100), (128, 0, 7)), ((100, 0, 1), (1, 7, 128))],
                         ids=["1tile_100x7", "1tile_1x128", "1tile_0x1", "1tile_100x0", "3tiles_a", "3tiles_b"])
def test_pair_counts_equal_numpy(gpu_required, side, counts, gts):
    rng = np.random.default_rng([side, len(counts), sum(gts)])
    D, cap, n = 100, 128, len(counts)
    det_p, det = _random_packed(rng, (n, D), side, 0.3)
    gt_p, gt = _random_packed(rng, (sum(gts),), side, 0.4)
    first = np.concatenate([[0], np.cumsum(gts)]).astype(np.int32)
    inter, d_area, g_area = pair_counts_device(det_p, np.array(counts, np.int32), gt_p, first, side, cap, prefill=-7)
    w_inter, w_d, w_g = np.zeros((n, D, cap), np.int32), np.zeros((n, D), np.int32), np.zeros((n, cap), np.int32)
    for t in range(n):
        c, g = counts[t], gts[t]
        dm = det[t, :c].reshape(c, side * side).astype(np.float64)    # 0/1 sums below 2^53: exact
        gm = gt[first[t]:first[t + 1]].reshape(g, side * side).astype(np.float64)
        w_inter[t, :c, :g] = dm @ gm.T
        w_d[t, :c] = dm.sum(1)
        w_g[t, :g] = gm.sum(1)
    assert np.array_equal(inter, w_inter) and np.array_equal(d_area, w_d) and np.array_equal(g_area, w_g)
    assert w_inter.any() == (any(c and g for c, g in zip(counts, gts)))


# ------------------------------------------------------------------------------------------------ engine
SMALL = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)
GT_PER_TILE = (5, 0, 9)


@pytest.fixture(scope="module")
def small(gpu_required):
    spec = EngineSpec(**SMALL)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 128, 128, 3, seed=77)
    eng = Engine(spec, W, (128, 128, 3), max_batch=3)
    polys, at = [], 0
    pool = family("inside", 128, sum(GT_PER_TILE), seed=5) + family("far", 128, 2, seed=5)
    for k in GT_PER_TILE:
        polys.append(pool[at:at + k])
        at += k
    polys[2] = polys[2][:-2] + pool[-2:]               # ground truth that leaves the tile, too
    ref = eng.infer(tiles)                             # the masks the counts are checked against: computed once
    assert sum(len(r) for r in ref) > 0 and any(r.pred_masks.any() for r in ref if len(r))
    yield spec, W, tiles, eng, polys, ref
    eng.close()


def _gt_masks(polys):
    box = np.array([0.0, 0.0, 128.0, 128.0])
    return np.stack([rasterize_polygons_within_box(p, box, 128) for p in polys]) if polys else np.zeros((0, 128, 128), bool)


def _check_tile(got, ref, polys):
    inst, inter, d_area, g_area = got
    assert np.array_equal(inst.pred_boxes.view(np.uint32), ref.pred_boxes.view(np.uint32))
    assert np.array_equal(inst.scores.view(np.uint32), ref.scores.view(np.uint32)) and np.array_equal(inst.pred_classes, ref.pred_classes)
    assert not inst.has("pred_masks")
    dm = ref.pred_masks.reshape(len(ref), 128 * 128).astype(np.float64)              # 0/1 sums below 2^53: exact
    gm = _gt_masks(polys).reshape(len(polys), 128 * 128).astype(np.float64)
    assert inter.shape == (len(ref), len(polys)) and inter.dtype == np.int32
    assert np.array_equal(inter, (dm @ gm.T).astype(np.int32))
    assert np.array_equal(d_area, dm.sum(1).astype(np.int32)) and np.array_equal(g_area, gm.sum(1).astype(np.int32))


@pytest.mark.parametrize("n", [3, 2], ids=["full_batch", "ragged_batch"])
def test_engine_counts_equal_counts_from_infer_masks(small, n):
    spec, W, tiles, eng, polys, ref = small
    before = eng.eval_fallbacks
    got = eng.eval_counts(tiles[:n], polys[:n])
    assert got is not None and len(got) == n and eng.eval_fallbacks == before
    ref_n = eng.infer(tiles[:n])                       # the same batch size: the convolutions' tile variants follow it
    for i in range(n):
        _check_tile(got[i], ref_n[i], polys[i])
    assert any(g[1].any() for g in got)


def test_engine_counts_of_a_forward_already_enqueued(small):
    spec, W, tiles, eng, polys, ref = small
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 3)
    got = eng.eval_counts(3, polys)
    for i in range(3):
        _check_tile(got[i], ref[i], polys[i])


def test_one_tile_path_eager_capture_replay(small):
    """n = 1 runs eagerly, is captured into a graph, and is replayed; the counts run behind it on the copy stream every time."""
    spec, W, tiles, eng, polys, ref = small
    got = [eng.eval_counts(tiles[:1], polys[:1]) for _ in range(3)]
    one = eng.infer(tiles[:1])[0]
    assert len(one) > 0
    for g in got:
        _check_tile(g[0], one, polys[0])


def test_match_records_of_the_two_routes_are_identical(small):
    spec, W, tiles, eng, polys, ref = small
    rng = np.random.default_rng(3)
    got = eng.eval_counts(tiles, polys)
    gts_m, dts_m, gts_c, dts_c = [], [], [], []
    for i in range(3):
        gm = _gt_masks(polys[i])
        boxes = np.array([[p[0][0::2].min(), p[0][1::2].min(), p[0][0::2].max(), p[0][1::2].max()] for p in polys[i]], np.float64).reshape(-1, 4)
        base = {"boxes": boxes, "classes": rng.integers(0, 2, len(polys[i])), "crowd": rng.random(len(polys[i])) < 0.2}
        inst, inter, d_area, g_area = got[i]
        gts_m.append(dict(base, masks=gm))
        gts_c.append(dict(base, mask_area=g_area))
        dts_m.append({"boxes": ref[i].pred_boxes, "classes": ref[i].pred_classes, "scores": ref[i].scores, "masks": ref[i].pred_masks})
        dts_c.append({"boxes": inst.pred_boxes, "classes": inst.pred_classes, "scores": inst.scores, "mask_inter": inter, "mask_area": d_area})
    for kind in ("segm", "bbox"):
        a = coco_eval.match_images(gts_m, dts_m, 2, kind, spec.detections_per_image)
        b = coco_eval.match_images(gts_c, dts_c, 2, kind, spec.detections_per_image)
        assert len(a) == len(b) == 3
        for ra, rb in zip(a, b):
            assert ra.keys() == rb.keys() and ra
            for k in ra:
                assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ra[k], rb[k])), (kind, k)


# ------------------------------------------------------------------------------------------------ fallback
def test_batches_beyond_the_pool_fall_back_and_leave_the_engine_usable(small):
    spec, W, tiles, eng, polys, ref = small
    before = eng.eval_fallbacks
    tri = [np.array([10.0, 10.0, 60.0, 12.0, 30.0, 70.0])]
    assert eng.eval_counts(tiles, [polys[0], [tri] * 129, polys[2]]) is None            # 129 ground truths in one tile
    assert eng.eval_fallbacks == before + 1
    a = np.linspace(0, 2 * np.pi, 15000, endpoint=False)
    ring = np.stack([64 + 50 * np.cos(a), 64 + 50 * np.sin(a)], 1).reshape(-1)          # 30000 doubles; 7 of them > 3 * 65536
    assert eng.eval_counts(tiles, [[[ring]] * 4, [[ring]] * 3, []]) is None
    assert eng.eval_fallbacks == before + 2
    fits = eng.eval_counts(tiles, [[[ring]] * 3, [[ring]] * 3, []])                    # 180000 doubles, 128-instance rule untouched: fits
    assert fits is not None and fits[0][1].shape[1] == 3
    got = eng.eval_counts(tiles, polys)                                                # a normal call afterwards
    for i in range(3):
        _check_tile(got[i], ref[i], polys[i])
    assert eng.eval_fallbacks == before + 2


def test_non_square_engine_falls_back(gpu_required):
    spec = EngineSpec(**SMALL)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (128, 160, 3), max_batch=1)
    try:
        assert eng.eval_counts(synthetic_tiles(1, 128, 160, 3, seed=1), [[[np.array([1.0, 1.0, 50.0, 1.0, 50.0, 50.0])]]]) is None
        assert eng.eval_fallbacks == 1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ command line
def _tiny_training_workdir(tmp_path):
    """The work directory of tests/test_gpu_trainer.py's CLI test, rebuilt: four 128 x 128 synthetic tiles with two boxes each, one
    training size, 3 iterations, evaluation at the third."""
    import yaml
    from PIL import Image

    wd = tmp_path / "outputs" / "obj_detector"
    (wd / "trn-images").mkdir(parents=True)
    tiles = synthetic_tiles(4, 128, 128, 3, seed=19)
    images, anns = [], []
    rng = np.random.default_rng(0)
    for i in range(4):
        fn = f"trn-images/18_{100 + i}_200.tif"
        Image.fromarray(tiles[i][:, :, ::-1]).save(str(wd / fn))
        images.append({"id": i, "file_name": fn, "width": 128, "height": 128})
        for j in range(2):
            x, y = rng.integers(5, 60, 2)
            w, h = rng.integers(20, 60, 2)
            anns.append({"id": len(anns), "image_id": i, "category_id": 1 + (j % 2), "bbox": [int(x), int(y), int(w), int(h)], "iscrowd": 0,
                         "segmentation": [[int(x), int(y), int(x + w), int(y), int(x + w), int(y + h), int(x), int(y + h)]], "area": int(w * h)})
    cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
    json.dump({"images": images, "annotations": anns, "categories": cats}, open(wd / "COCO_trn.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320, "RANDOM_FLIP": "horizontal", "MIN_SIZE_TRAIN": [192]},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200, "BATCH_SIZE_PER_IMAGE": 64}, "ROI_HEADS": {"NUM_CLASSES": 2, "BATCH_SIZE_PER_IMAGE": 64}},
          "SOLVER": {"BASE_LR": 0.002, "IMS_PER_BATCH": 2, "MAX_ITER": 3, "WARMUP_ITERS": 2, "STEPS": [2], "GAMMA": 0.5, "CHECKPOINT_PERIOD": 3},
          "TEST": {"DETECTIONS_PER_IMAGE": 20, "EVAL_PERIOD": 3}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"train_model.py": {"working_directory": str(wd), "log_subfolder": "logs", "COCO_files": {"trn": "COCO_trn.json", "val": "COCO_trn.json"},
                              "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {}}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return wd


def test_cli_device_evaluation_lines_equal_host(gpu_required, tmp_path, caplog):
    from proj_roadsurf_amd import train_model
    cwd = os.getcwd()
    evals = {}
    try:
        for mode in ("device", "host"):
            root = tmp_path / mode
            root.mkdir()
            wd = _tiny_training_workdir(root)
            with caplog.at_level(logging.INFO, logger="train_model"):
                caplog.clear()
                assert train_model.main([str(root / "config.yaml"), "--synthetic-weights", "--log-period", "1", "--loss-scale", "256", "--precision", "fp16",
                                         "--tagged-samples", "0", "--val-ap", mode]) == 0
                text = caplog.text
            os.chdir(cwd)
            lines = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
            assert [("validation_loss" in l) for l in lines] == [False, False, True]
            evals[mode] = {k: v for k, v in lines[-1].items() if k.startswith(("bbox/", "segm/"))}
            if mode == "device":
                assert "val_ap: 0 chunks evaluated on the host" in text
            else:
                assert "val_ap:" not in text
    finally:
        os.chdir(cwd)
    print(evals)
    assert "bbox/AP" in evals["host"] and "segm/AP" in evals["host"]
    assert evals["device"] == evals["host"]
