"""``make_detections --vote-geometry polygons`` end to end on the two small datasets of tests/test_gpu_road_metrics_cli.py: the JSON
files carry the key and the host route's roads, the switch is refused without ``--vectorize device``, the default geometry's files
do not change by a byte, and two ranks write the one-rank files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from proj_roadsurf_amd import raster_vote as RV
from tests.test_gpu_road_metrics_cli import BATCH, ROOT, SETS, TILE, _dataset, _dump, GPKG

pytestmark = pytest.mark.gpu


def _files(wd):
    out = {n: (open(wd / f"{n}_road_votes.json", "rb").read(), _dump(str(wd / (GPKG.format(n) + ".gpkg")))) for n in SETS}
    out["metrics"] = open(wd / "road_metrics.json", "rb").read()
    return out


def _expected_roads(tmp_path, wd, docs, threshold):
    """The road table of every dataset through the host route: the CLI's engine and batches, polygons fetched with the CLI's epsilon."""
    from proj_roadsurf_amd.decode_pool import read_tile
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import load_d2_yaml
    from proj_roadsurf_amd.weights import synthetic_weights
    spec = load_d2_yaml(str(tmp_path / "d2.yaml"), num_classes=2).replace(score_thresh_test=0.05)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (TILE, TILE, 3), max_batch=BATCH)
    out = {}
    try:
        for name, (images, anns) in docs.items():
            tiles = np.stack([read_tile(str(wd / e["file_name"])) for e in images])
            res = []
            for i in range(0, len(images), BATCH):
                eng.infer_device(eng.upload_async(np.ascontiguousarray(tiles[i:i + BATCH])), len(tiles[i:i + BATCH]))
                eng.fetch_async(len(tiles[i:i + BATCH]), polygons=True, rdp_epsilon=0.75, masks=True)
                res += eng.fetch_wait(len(tiles[i:i + BATCH]))
            labels = [[[np.array(r) for r in a["segmentation"]] for a in anns if a["image_id"] == e["id"]] for e in images]
            ids = [[a.get("road_id", a["id"]) for a in anns if a["image_id"] == e["id"]] for e in images]
            rows = eng.polygon_vote_host_rows(res, labels, [threshold])
            out[name] = RV.reduce_votes([RV.sweep_slice(r, 0) for r in rows], ids, {0: "artificial", 1: "natural"})
    finally:
        eng.close()
    return out


def test_vote_geometry_switch(gpu_required, tmp_path):
    from proj_roadsurf_amd import make_detections
    cfg, wd, docs = _dataset(tmp_path)
    common = [cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0", "--road-votes", "--road-metrics"]
    cwd = os.getcwd()
    try:
        for bad in (common + ["--vote-geometry", "polygons"], common + ["--vote-geometry", "polygons", "--vectorize", "host"],
                    common[:6] + ["--vectorize", "device", "--vote-geometry", "polygons"]):
            with pytest.raises(SystemExit):
                make_detections.main(bad)
            os.chdir(cwd)
        assert not (wd / "val_road_votes.json").exists()                                   # refused up front: nothing ran
        assert make_detections.main(common + ["--vectorize", "device"]) == 0
        os.chdir(cwd)
        plain = _files(wd)
        assert make_detections.main(common + ["--vectorize", "device", "--vote-geometry", "polygons"]) == 0
        os.chdir(cwd)
        poly = _files(wd)
        assert make_detections.main(common + ["--vectorize", "device"]) == 0               # and the default again: byte for byte
        os.chdir(cwd)
        again = _files(wd)
        assert make_detections.main(common + ["--vectorize", "device", "--vote-geometry", "pixels"]) == 0
        os.chdir(cwd)
        named = _files(wd)
    finally:
        os.chdir(cwd)
    assert again == plain and named == plain
    assert b"geometry" not in plain["metrics"] and all(b"geometry" not in plain[n][0] for n in SETS)
    want = _expected_roads(tmp_path, wd, docs, 0.3)
    for n in SETS:
        doc = json.loads(poly[n][0])
        assert doc["geometry"] == "polygons" and doc["roads"] == json.loads(json.dumps(want[n])) and len(doc["roads"]) > 0
        assert isinstance(json.loads(plain[n][0]), list)
        assert poly[n][1] == plain[n][1]                                                    # the GeoPackage does not depend on the vote
    m = json.loads(poly["metrics"])
    assert m["geometry"] == "polygons" and len(m["sweep"]) == 20
    assert {k: v for k, v in m.items() if k != "geometry"}.keys() == json.loads(plain["metrics"]).keys()


def test_two_ranks_write_the_one_rank_files(gpu_required, tmp_path):
    cfg, wd, docs = _dataset(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT, RS_DIST_BACKEND="gloo")
    common = ["-m", "proj_roadsurf_amd.make_detections", cfg, "--synthetic-weights", "--batch", str(BATCH), "--tagged-samples", "0", "--road-votes",
              "--road-metrics", "--vectorize", "device", "--vote-geometry", "polygons"]
    r1 = subprocess.run([sys.executable] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stderr[-3000:]
    one = {n: open(wd / n, "rb").read() for n in ("road_metrics.json", "val_road_votes.json", "tst_road_votes.json")}
    for n in one:
        os.remove(wd / n)
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", "29647"] + common, env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stderr[-3000:]
    assert {n: open(wd / n, "rb").read() for n in one} == one
    assert json.loads(one["road_metrics.json"])["geometry"] == "polygons" and json.loads(one["val_road_votes.json"])["geometry"] == "polygons"
