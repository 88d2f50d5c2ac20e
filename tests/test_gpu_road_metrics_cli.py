"""``make_detections --road-metrics`` end to end on two small synthetic datasets, ``val`` and ``tst``: the ``road_metrics.json`` it
writes is the one ``road_metrics.report`` gives on ``vote_tables_host(..., thresholds=)`` of the same detections, every other output
is what it is without the switch, and two ranks write the one-rank file."""
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from proj_roadsurf_amd import road_metrics as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE, BATCH = 128, 2
SETS = {"val": 4, "tst": 3}                                     # tiles per dataset: tst ends on a ragged batch
GPKG = "{}_detections_at_0dot05_threshold"


def _rect(x0, y0, x1, y1):
    return [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]


def _dataset(tmp_path):
    """The working directory of tests/test_gpu_road_votes_cli.py with two datasets.  Road "A" (artificial) crosses val tiles 0..2,
    "X" (natural) lies in val tile 3 and in tst tile 0, every tile has a road of its own whose category alternates."""
    import yaml
    from PIL import Image
    from tests.util import synthetic_tiles
    wd = tmp_path / "outputs" / "obj_detector"
    cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
    tiles = synthetic_tiles(sum(SETS.values()), TILE, TILE, 3, seed=9)
    docs, k = {}, 0
    for name, n in SETS.items():
        (wd / f"{name}-images").mkdir(parents=True)
        images, anns = [], []

        def ann(image, seg, category, **kw):
            anns.append(dict({"id": 100 * (1 + len(docs)) + len(anns), "image_id": image, "category_id": category, "segmentation": seg, "iscrowd": 0}, **kw))
        for i in range(n):
            fn = f"{name}-images/18_{100 + k}_200.tif"
            Image.fromarray(tiles[k][:, :, ::-1]).save(str(wd / fn))
            images.append({"id": i, "file_name": fn, "width": TILE, "height": TILE})
            if name == "val" and i <= 2:
                ann(i, [_rect(0, 20, 128, 70)], 1, road_id="A")
            if (name, i) in (("val", 3), ("tst", 0)):
                ann(i, [_rect(40.5, 0, 100, 128)], 2, road_id="X")
            ann(i, [_rect(10, 60, 120, 125.5)], 1 + k % 2)
            k += 1
        docs[name] = (images, anns)
        json.dump({"images": images, "annotations": anns, "categories": cats}, open(wd / f"COCO_{name}.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200}, "ROI_HEADS": {"NUM_CLASSES": 1}},
          "TEST": {"DETECTIONS_PER_IMAGE": 20}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"make_detections.py": {"working_directory": str(wd), "log_subfolder": "logs", "COCO_files": {n: f"COCO_{n}.json" for n in SETS},
                                  "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {"pth_file": "logs/model_0005999.pth"},
                                  "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05},
           "determine_class.py": {"threshold": 0.3}, "final_metrics.py": {"baseline": "all natural"}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"), sort_keys=False)      # COCO_files in the order val, tst: the dataset order
    return str(tmp_path / "config.yaml"), wd, docs


def _expected(tmp_path, wd, docs, thresholds):
    """The document from fetched masks: the CLI's engine and batches, the numpy route per threshold, the metrics on the host."""
    from proj_roadsurf_amd.decode_pool import read_tile
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import load_d2_yaml
    from proj_roadsurf_amd.weights import synthetic_weights
    spec = load_d2_yaml(str(tmp_path / "d2.yaml"), num_classes=2).replace(score_thresh_test=0.05)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (TILE, TILE, 3), max_batch=BATCH)
    sets, categories = {}, {}
    try:
        for name, (images, anns) in docs.items():
            tiles = np.stack([read_tile(str(wd / e["file_name"])) for e in images])
            dets = [r for i in range(0, len(images), BATCH) for r in eng.infer(tiles[i:i + BATCH])]
            labels = [[[np.array(r) for r in a["segmentation"]] for a in anns if a["image_id"] == e["id"]] for e in images]
            ids = [[a.get("road_id", a["id"]) for a in anns if a["image_id"] == e["id"]] for e in images]
            sets[name] = (ids, [t[:3] for t in RV.vote_tables_host(dets, labels, 2, thresholds=thresholds)])
            for a in anns:
                categories.setdefault(a.get("road_id", a["id"]), {1: "artificial", 2: "natural"}[a["category_id"]])
    finally:
        eng.close()
    return M.report(sets, categories, ["artificial", "natural"], thresholds, baseline_class="natural")


def _dump(path):
    """Every table of a GeoPackage, row for row and blob for blob, without gpkg_contents.last_change (the wall clock of the write)."""
    con = sqlite3.connect(path)
    try:
        out = {"schema": con.execute("SELECT type, name, tbl_name, sql FROM sqlite_master ORDER BY name").fetchall()}
        for (t,) in con.execute("SELECT name FROM sqlite_master WHERE type = 'table' ORDER BY name").fetchall():
            cols = [c[1] for c in con.execute(f'PRAGMA table_info("{t}")').fetchall() if c[1] != "last_change"]
            out[t] = con.execute('SELECT %s FROM "%s" ORDER BY rowid' % (", ".join(f'"{c}"' for c in cols), t)).fetchall()
        return out
    finally:
        con.close()


def _outputs(wd):
    return {n: (open(wd / f"{n}_road_votes.json", "rb").read(), _dump(str(wd / (GPKG.format(n) + ".gpkg")))) for n in SETS}


def test_road_metrics_switch_writes_the_host_document_and_leaves_the_rest(gpu_required, tmp_path):
    from proj_roadsurf_amd import make_detections
    cfg, wd, docs = _dataset(tmp_path)
    want = _expected(tmp_path, wd, docs, M.REFERENCE_THRESHOLDS)
    common = [cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0"]
    cwd = os.getcwd()
    try:
        assert make_detections.main(common + ["--road-votes"]) == 0
        os.chdir(cwd)
        assert not (wd / "road_metrics.json").exists()
        plain = _outputs(wd)
        assert make_detections.main(common + ["--road-votes", "--road-metrics"]) == 0       # the sweep carries the vote's threshold
        os.chdir(cwd)
        both = json.load(open(wd / "road_metrics.json"))
        assert _outputs(wd) == plain and all(len(plain[n][1][GPKG.format(n)]) > 0 for n in SETS)
        os.remove(wd / "road_metrics.json")
        assert make_detections.main(common + ["--road-metrics"]) == 0                       # and the switch alone
        os.chdir(cwd)
        got = json.load(open(wd / "road_metrics.json"))
        assert make_detections.main(common + ["--road-metrics", "--metric-thresholds", "0.5,0,0.25"]) == 0
    finally:
        os.chdir(cwd)
    assert got == json.loads(json.dumps(want)) == both
    assert got["thresholds"] == [float(t) for t in M.REFERENCE_THRESHOLDS] and got["sweep_on"] == "val" and len(got["sweep"]) == 20
    assert list(got["datasets"])[:4] == ["all datasets", "val", "tst", "training zone"] and got["baseline"]["class"] == "natural"
    assert sum(c["TP"] + c["FP"] for c in got["sweep"][0]["by_class"]) >= 2, got["sweep"][0]          # the labels meet detections
    assert sum(c["count"] for c in got["datasets"]["all datasets"]["by_class"]) == 9                  # A, X and seven roads of their own
    assert sum(c["count"] for c in got["datasets"]["val"]["by_class"]) == 6 and sum(c["count"] for c in got["datasets"]["tst"]["by_class"]) == 4
    three = json.load(open(wd / "road_metrics.json"))
    assert three == json.loads(json.dumps(_expected(tmp_path, wd, docs, [0.5, 0.0, 0.25]))) and three["thresholds"] == [0.5, 0.0, 0.25]
    for bad in (["--metric-thresholds", ",".join(["0.1"] * 33)], ["--metric-thresholds", "0.1,x"]):
        with pytest.raises(SystemExit):
            make_detections.main(common + ["--road-metrics"] + bad)
        os.chdir(cwd)


def test_two_ranks_write_the_one_rank_metrics(gpu_required, tmp_path):
    cfg, wd, docs = _dataset(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, RS_DIST_BACKEND="gloo")
    common = ["-m", "proj_roadsurf_amd.make_detections", cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0", "--road-metrics"]
    r1 = subprocess.run([sys.executable] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = open(wd / "road_metrics.json", "rb").read()
    os.remove(wd / "road_metrics.json")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", "29643"] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert open(wd / "road_metrics.json", "rb").read() == one and len(json.loads(one)["sweep"]) == 20
    assert "0 of 4 batches were voted on the host" in r1.stderr and "0 of 4 batches were voted on the host" in r2.stderr
