"""``make_detections --road-votes`` end to end on a small synthetic tileset: the road table it writes is the one
``reduce_votes(vote_tables_host(...))`` gives for the same detections, every other output is what it is without the switch, and two
ranks write the one-rank file."""
import json
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "val_detections_at_0dot05_threshold"
N_TILES, TILE, BATCH, THRESHOLD = 6, 128, 4, 0.3


def _rect(x0, y0, x1, y1):
    return [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]


def _dataset(tmp_path):
    """The working directory of tests/test_vector_cli.py with road labels as polygon annotations: road "A" crosses tiles 0..2, "B"
    tiles 2..4, every tile has a road of its own (named by the annotation's id: no road_id), tile 5 a label of two rings; one crowd and
    one RLE annotation are no labels.  The YAML carries determine_class.py's threshold."""
    import yaml
    from PIL import Image
    from tests.util import synthetic_tiles
    wd = tmp_path / "outputs" / "obj_detector"
    (wd / "val-images").mkdir(parents=True)
    tiles = synthetic_tiles(N_TILES, TILE, TILE, 3, seed=9)
    images, anns = [], []

    def ann(image, seg, **kw):
        anns.append(dict({"id": 100 + len(anns), "image_id": image, "category_id": 1, "segmentation": seg, "iscrowd": 0}, **kw))
    for i in range(N_TILES):
        fn = f"val-images/18_{100 + i}_200.tif"
        Image.fromarray(tiles[i][:, :, ::-1]).save(str(wd / fn))
        images.append({"id": i, "file_name": fn, "width": TILE, "height": TILE})
        if i <= 2:
            ann(i, [_rect(0, 20, 128, 70)], road_id="A")
        if 2 <= i <= 4:
            ann(i, [_rect(40.5, 0, 100, 128)], road_id="B")
        ann(i, [_rect(10, 60, 120, 125.5)])
    ann(5, [_rect(0, 0, 60, 60), _rect(64, 64, 128, 128)], road_id="two_rings")
    ann(1, [_rect(0, 0, 128, 128)], road_id="crowd", iscrowd=1)
    ann(3, {"size": [TILE, TILE], "counts": "abc"}, road_id="rle")
    cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
    json.dump({"images": images, "annotations": anns, "categories": cats}, open(wd / "COCO_val.json", "w"))
    d2 = {"INPUT": {"FORMAT": "RGB", "MIN_SIZE_TEST": 192, "MAX_SIZE_TEST": 320},
          "MODEL": {"RPN": {"PRE_NMS_TOPK_TEST": 200, "POST_NMS_TOPK_TEST": 200}, "ROI_HEADS": {"NUM_CLASSES": 1}},
          "TEST": {"DETECTIONS_PER_IMAGE": 20}}
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cfg = {"make_detections.py": {"working_directory": str(wd), "log_subfolder": "logs", "COCO_files": {"val": "COCO_val.json"},
                                  "detectron2_config_file": str(tmp_path / "d2.yaml"), "model_weights": {"pth_file": "logs/model_0005999.pth"},
                                  "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05},
           "determine_class.py": {"threshold": THRESHOLD}}
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return str(tmp_path / "config.yaml"), wd, images, anns


def _expected(tmp_path, wd, images, anns):
    """The road table from fetched masks: the CLI's engine, its batches, the numpy route, the reduction."""
    from proj_roadsurf_amd.decode_pool import read_tile
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import load_d2_yaml
    from proj_roadsurf_amd.weights import synthetic_weights
    spec = load_d2_yaml(str(tmp_path / "d2.yaml"), num_classes=2).replace(score_thresh_test=0.05)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (TILE, TILE, 3), max_batch=BATCH)
    try:
        tiles = np.stack([read_tile(str(wd / e["file_name"])) for e in images])
        dets = [r for i in range(0, N_TILES, BATCH) for r in eng.infer(tiles[i:i + BATCH])]
    finally:
        eng.close()
    labels, ids = [], []
    for e in images:
        mine = [a for a in anns if a["image_id"] == e["id"] and not a["iscrowd"] and isinstance(a["segmentation"], list)]
        labels.append([[np.array(r) for r in a["segmentation"]] for a in mine])
        ids.append([a.get("road_id", a["id"]) for a in mine])
    return RV.reduce_votes(RV.vote_tables_host(dets, labels, 2, THRESHOLD), ids), dets


def _dump(path):
    """Every table of a GeoPackage, row for row and blob for blob, without gpkg_contents.last_change (the wall clock of the write: two
    runs of the same command differ there, so the files' raw bytes cannot be compared)."""
    con = sqlite3.connect(path)
    try:
        out = {"schema": con.execute("SELECT type, name, tbl_name, sql FROM sqlite_master ORDER BY name").fetchall()}
        for (t,) in con.execute("SELECT name FROM sqlite_master WHERE type = 'table' ORDER BY name").fetchall():
            cols = [c[1] for c in con.execute(f'PRAGMA table_info("{t}")').fetchall() if c[1] != "last_change"]
            out[t] = con.execute('SELECT %s FROM "%s" ORDER BY rowid' % (", ".join(f'"{c}"' for c in cols), t)).fetchall()
        return out
    finally:
        con.close()


def test_road_votes_switch_writes_the_host_table_and_leaves_the_rest(gpu_required, tmp_path):
    from proj_roadsurf_amd import make_detections
    cfg, wd, images, anns = _dataset(tmp_path)
    want, dets = _expected(tmp_path, wd, images, anns)
    common = [cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0", "--geojson"]
    cwd = os.getcwd()
    try:
        assert make_detections.main(common) == 0
        os.chdir(cwd)
        assert not (wd / "val_road_votes.json").exists()
        plain, plain_json = _dump(str(wd / f"{NAME}.gpkg")), open(wd / f"{NAME}.geojson", "rb").read()
        assert make_detections.main(common + ["--road-votes"]) == 0
    finally:
        os.chdir(cwd)
    got = json.load(open(wd / "val_road_votes.json"))
    assert got == want
    by = {g["road_id"]: g for g in got}
    assert [g["road_id"] for g in got] == ["A", 101, 103, "B", 106, 108, 110, 111, "two_rings"] and "crowd" not in by and "rle" not in by
    assert sum(g["cover_type"] != "undetected" for g in got) >= 3, got        # the labels meet detections
    assert _dump(str(wd / f"{NAME}.gpkg")) == plain and len(plain[NAME]) > N_TILES
    assert open(wd / f"{NAME}.geojson", "rb").read() == plain_json
    # the YAML's threshold was the default; the switch for it wins
    cwd = os.getcwd()
    try:
        assert make_detections.main(common + ["--road-votes", "--vote-threshold", "0"]) == 0
    finally:
        os.chdir(cwd)
    labels = [[[np.array(r) for r in a["segmentation"]] for a in anns if a["image_id"] == e["id"] and not a["iscrowd"] and isinstance(a["segmentation"], list)]
              for e in images]
    ids = [[a.get("road_id", a["id"]) for a in anns if a["image_id"] == e["id"] and not a["iscrowd"] and isinstance(a["segmentation"], list)] for e in images]
    assert json.load(open(wd / "val_road_votes.json")) == RV.reduce_votes(RV.vote_tables_host(dets, labels, 2, 0.0), ids)


def test_two_ranks_write_the_one_rank_road_table(gpu_required, tmp_path):
    cfg, wd, images, anns = _dataset(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, RS_DIST_BACKEND="gloo")
    common = ["-m", "proj_roadsurf_amd.make_detections", cfg, "--synthetic-weights", "--batch", "2", "--tagged-samples", "0", "--road-votes"]
    r1 = subprocess.run([sys.executable] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = open(wd / "val_road_votes.json", "rb").read()
    one_gpkg = _dump(str(wd / f"{NAME}.gpkg"))
    os.remove(wd / "val_road_votes.json")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", "29641"] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert open(wd / "val_road_votes.json", "rb").read() == one and len(json.loads(one)) == 9
    assert _dump(str(wd / f"{NAME}.gpkg")) == one_gpkg
    assert "0 of 3 batches were voted on the host" in r1.stderr and "0 of 4 batches were voted on the host" in r2.stderr
