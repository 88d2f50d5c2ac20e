"""COCOeval's evaluateImg on the GPU (csrc/val_ap.hip coco_order_kernel / coco_match_kernel, ``rs_op_coco_match``,
``Engine.eval_matches``, ``train_model --val-ap device-match``): the operator against the host restatement table for table and against
``coco_eval.match_images`` record for record on every case of tests/coco_match_cases.py, the engine's records against those matched on
the host from ``eval_counts``' tables and from ``infer()``'s masks, the fallbacks, and the command line.  Every comparison is exact."""
import json
import logging
import os

import numpy as np
import pytest

from proj_roadsurf_amd import coco_eval, coco_match
from proj_roadsurf_amd.engine import Engine
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.train_targets import rasterize_polygons_within_box
from proj_roadsurf_amd.weights import synthetic_weights
from tests import coco_match_cases as M
from tests.util import synthetic_tiles
from tests.val_ap_cases import family

pytestmark = pytest.mark.gpu
KINDS = ("bbox", "segm")


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("name", M.NAMES)
def test_operator_equals_host_restatement_and_match_images(gpu_required, name):
    b = M.case(name)
    want = coco_match.host_tables(b)
    first = coco_match.device_tables(b, prefill=-7)
    second = coco_match.device_tables(b, prefill=0x55555555)         # whatever the buffers held: every entry is written
    for k in coco_match.TABLES:
        assert first[k].tobytes() == second[k].tobytes(), k
        assert np.array_equal(first[k], want[k]), (k, int((first[k] != want[k]).sum()))
    for kind in KINDS:
        assert M.records_equal(coco_match.records(b, first, kind), M.reference(name, kind))


# ------------------------------------------------------------------------------------------------ engine
SMALL = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)
GT_PER_TILE = (5, 0, 9)
BOX = np.array([0.0, 0.0, 128.0, 128.0])


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
    rng = np.random.default_rng(3)
    classes = [rng.integers(0, 2, len(img)) for img in polys]
    # random weights put no detection on a star: tiles 0 and 2 also get the rectangles of their own first detections as ground truth, in
    # the detections' categories, so that the records hold matches (tile 1 stays empty)
    for i, r in enumerate(eng.infer(tiles)):
        if i != 1:
            for (x0, y0, x1, y1), c in zip(r.pred_boxes[:4].astype(np.float64), r.pred_classes[:4]):
                polys[i].append([np.array([x0, y0, x1, y0, x1, y1, x0, y1])])
                classes[i] = np.append(classes[i], c)
    boxes = [np.array([[p[0][0::2].min(), p[0][1::2].min(), p[0][0::2].max(), p[0][1::2].max()] for p in img], np.float64).reshape(-1, 4) for img in polys]
    gt_masks = [np.stack([rasterize_polygons_within_box(p, BOX, 128) for p in img]) if img else np.zeros((0, 128, 128), bool) for img in polys]
    want = {}                                          # per batch size (the convolutions' tile variants follow it): references, once

    def reference(n):
        if n not in want:
            ref = eng.infer(tiles[:n])
            counted = eng.eval_counts(tiles[:n], polys[:n])
            gts_m = [{"boxes": boxes[i], "classes": classes[i], "masks": gt_masks[i]} for i in range(n)]
            dts_m = [{"boxes": r.pred_boxes, "classes": r.pred_classes, "scores": r.scores, "masks": r.pred_masks} for r in ref]
            gts_c = [{"boxes": boxes[i], "classes": classes[i], "mask_area": counted[i][3]} for i in range(n)]
            dts_c = [{"boxes": c[0].pred_boxes, "classes": c[0].pred_classes, "scores": c[0].scores, "mask_inter": c[1], "mask_area": c[2]} for c in counted]
            D = spec.detections_per_image
            want[n] = (ref, {k: coco_eval.match_images(gts_m, dts_m, 2, k, D) for k in KINDS}, {k: coco_eval.match_images(gts_c, dts_c, 2, k, D) for k in KINDS})
        return want[n]
    full = reference(3)
    assert sum(len(r) for r in full[0]) > 0 and any(r.pred_masks.any() for r in full[0] if len(r))
    hits = {k: sum(int(rec[key][1][0].sum()) for rec in full[1][k] for key in rec if key[1] == "all") for k in KINDS}
    print(f"engine fixture: {[len(r) for r in full[0]]} detections, {[len(c) for c in classes]} ground truths, matched at IoU 0.5: {hits}")
    assert hits["bbox"] >= 2      # the rectangles at least; what the random-weight masks reach of them is printed, not required
    yield spec, tiles, eng, polys, boxes, classes, reference
    eng.close()


def _check(got, n, reference):
    ref, from_masks, from_counts = reference(n)
    assert got is not None and len(got) == n
    for i, (inst, rb, rs) in enumerate(got):
        assert np.array_equal(inst.pred_boxes.view(np.uint32), ref[i].pred_boxes.view(np.uint32))
        assert np.array_equal(inst.scores.view(np.uint32), ref[i].scores.view(np.uint32)) and np.array_equal(inst.pred_classes, ref[i].pred_classes)
        assert not inst.has("pred_masks")
    for kind, col in (("bbox", 1), ("segm", 2)):
        assert M.records_equal([g[col] for g in got], from_counts[kind])
        assert M.records_equal([g[col] for g in got], from_masks[kind])


@pytest.mark.parametrize("n", [3, 2], ids=["full_batch", "ragged_batch"])
def test_engine_records_equal_host_matching(small, n):
    spec, tiles, eng, polys, boxes, classes, reference = small
    before = eng.eval_fallbacks
    _check(eng.eval_matches(tiles[:n], boxes[:n], classes[:n], polys[:n]), n, reference)
    assert eng.eval_fallbacks == before


def test_engine_records_of_a_forward_already_enqueued(small):
    spec, tiles, eng, polys, boxes, classes, reference = small
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles)), 3)
    _check(eng.eval_matches(3, boxes, classes, polys), 3, reference)


def test_one_tile_path_eager_capture_replay(small):
    """n = 1 runs eagerly, is captured into a graph, and is replayed; the matching runs behind it on the copy stream every time."""
    spec, tiles, eng, polys, boxes, classes, reference = small
    for _ in range(3):
        _check(eng.eval_matches(tiles[:1], boxes[:1], classes[:1], polys[:1]), 1, reference)
    assert len(reference(1)[0][0]) > 0


def test_records_taken_while_the_next_forward_runs(small):
    """A second forward (other tiles) is enqueued directly behind the fetch, before anybody waits: the records are those of the first."""
    spec, tiles, eng, polys, boxes, classes, reference = small
    assert eng.eval_matches(tiles, boxes, classes, polys, wait=False) is True
    eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles[::-1])), 3)
    _check(eng.eval_matches_wait(3), 3, reference)
    eng.sync()
    _check(eng.eval_matches(tiles, boxes, classes, polys), 3, reference)


# ------------------------------------------------------------------------------------------------ fallback
def test_batches_beyond_the_pool_fall_back_and_leave_the_engine_usable(small):
    spec, tiles, eng, polys, boxes, classes, reference = small
    before = eng.eval_fallbacks
    tri = [np.array([10.0, 10.0, 60.0, 12.0, 30.0, 70.0])]
    many_b, many_c = np.tile([10.0, 10.0, 60.0, 70.0], (129, 1)), np.zeros(129, np.int64)
    assert eng.eval_matches(tiles, [boxes[0], many_b, boxes[2]], [classes[0], many_c, classes[2]], [polys[0], [tri] * 129, polys[2]]) is None
    assert eng.eval_fallbacks == before + 1
    _check(eng.eval_matches(tiles, boxes, classes, polys), 3, reference)           # the next fitting batch
    assert eng.eval_fallbacks == before + 1
    with pytest.raises(ValueError):
        eng.eval_matches(tiles, boxes[:2], classes, polys)


def test_non_square_engine_falls_back(gpu_required):
    spec = EngineSpec(**SMALL)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (128, 160, 3), max_batch=1)
    try:
        got = eng.eval_matches(synthetic_tiles(1, 128, 160, 3, seed=1), [np.array([[1.0, 1.0, 50.0, 50.0]])], [np.array([0])],
                               [[[np.array([1.0, 1.0, 50.0, 1.0, 50.0, 50.0])]]])
        assert got is None and eng.eval_fallbacks == 1
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ command line
def _tiny_training_workdir(tmp_path, oversized):
    """The work directory of tests/test_gpu_val_ap.py's CLI test, rebuilt: four 128 x 128 synthetic tiles with two boxes each, one
    training size, 3 iterations, evaluation at the third.  The validation set is a file of its own; ``oversized`` gives its first
    image an annotation of 1500 polygons, more than the device pool of a two-image chunk holds (1024)."""
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
    val = [dict(a) for a in anns]
    if oversized:
        val[0]["segmentation"] = val[0]["segmentation"] * 1500
    json.dump({"images": images, "annotations": val, "categories": cats}, open(wd / "COCO_val.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320, "RANDOM_FLIP": "horizontal", "MIN_SIZE_TRAIN": [192]},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200, "BATCH_SIZE_PER_IMAGE": 64}, "ROI_HEADS": {"NUM_CLASSES": 2, "BATCH_SIZE_PER_IMAGE": 64}},
          "SOLVER": {"BASE_LR": 0.002, "IMS_PER_BATCH": 2, "MAX_ITER": 3, "WARMUP_ITERS": 2, "STEPS": [2], "GAMMA": 0.5, "CHECKPOINT_PERIOD": 3},
          "TEST": {"DETECTIONS_PER_IMAGE": 20, "EVAL_PERIOD": 3}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"train_model.py": {"working_directory": str(wd), "log_subfolder": "logs", "COCO_files": {"trn": "COCO_trn.json", "val": "COCO_val.json"},
                              "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {}}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return wd


@pytest.mark.parametrize("oversized,fallbacks", [(False, 0), (True, 1)], ids=["fits", "one_oversized_image"])
def test_cli_device_match_lines_equal_host(gpu_required, tmp_path, caplog, oversized, fallbacks):
    from proj_roadsurf_amd import train_model
    cwd = os.getcwd()
    evals = {}
    try:
        for mode in ("device-match", "host"):
            root = tmp_path / mode
            root.mkdir()
            wd = _tiny_training_workdir(root, oversized)
            with caplog.at_level(logging.INFO, logger="train_model"):
                caplog.clear()
                assert train_model.main([str(root / "config.yaml"), "--synthetic-weights", "--log-period", "1", "--loss-scale", "256", "--precision", "fp16",
                                         "--tagged-samples", "0", "--val-ap", mode]) == 0
                text = caplog.text
            os.chdir(cwd)
            lines = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
            assert [("validation_loss" in l) for l in lines] == [False, False, True]
            evals[mode] = {k: v for k, v in lines[-1].items() if k.startswith(("bbox/", "segm/"))}
            if mode == "device-match":
                assert f"val_ap: {fallbacks} chunks evaluated on the host" in text
            else:
                assert "val_ap:" not in text
    finally:
        os.chdir(cwd)
    print(evals)
    assert "bbox/AP" in evals["host"] and "segm/AP" in evals["host"] and len(evals["host"]) == 2 * (6 + 2)
    assert evals["device-match"] == evals["host"]
