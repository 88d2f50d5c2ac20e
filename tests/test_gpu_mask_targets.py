"""Mask-head training targets rasterised on the GPU (csrc/mask_targets.h + mask_targets_kernel, ``Trainer(mask_targets="device")``,
``train_model.py --mask-targets device``) against the host rasteriser they replace.  The feature's claim is identical bits, so every
comparison is ``np.array_equal``: the operator on polygon families built to reach each rule of the closed form, a whole training
step in both precisions, the capacity fallback, the argument error and the command-line tool."""
import json
import os

import numpy as np
import pytest

from proj_roadsurf_amd.engine import Trainer
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.train_targets import rasterize_entries, rasterize_entries_device
from proj_roadsurf_amd.weights import synthetic_weights
from tests.mask_target_cases import FAMILIES, ORACLE_FAMILIES, family, mixed
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu

S = 28
# entries per family call: the "far" family costs the HOST reference about 10^6 boundary points per edge, so it stays small
FAMILY_ENTRIES = {"far": 64, "long": 96}
NAMES = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")


def _compare(instances, ent, boxes):
    want = rasterize_entries(instances, ent, boxes, S)
    got = rasterize_entries_device(instances, ent, boxes, S)
    assert got.shape == want.shape == (len(ent), S, S)
    differing = [int(e) for e in np.nonzero((got != want).reshape(len(ent), S * S).any(1))[0]]
    assert not differing, f"{len(differing)} of {len(ent)} masks differ from the host's, first entries {differing[:8]}"
    assert np.array_equal(got, want)
    return want


@pytest.mark.parametrize("name", FAMILIES)
def test_operator_equals_host_per_family(gpu_required, name):
    """One call per family (tests/mask_target_cases.py): inside the box; +-1000 px around boxes 0.05..3 px wide (the max(., 0.1)
    branch, scaled coordinates of 10^6); the 5x grid and its half steps at ratio exactly 1; integer vertices (axis-aligned, 45 degree,
    the dx == dy tie); repeated vertices and collinear triples; unions with a hole ring; several hundred vertices."""
    n = FAMILY_ENTRIES.get(name, 256)
    instances, ent, boxes = family(name, n, seed=3)
    want = _compare(instances, ent, boxes)
    fill = float(want.mean())
    print(f"{name}: {n} entries, {sum(len(p) for p in instances)} polygons, foreground {fill:.3f}")
    assert 0.01 < fill < 0.99, "the family does not exercise the rasteriser"


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 2 * 256])
def test_operator_equals_host_per_entry_count(gpu_required, count):
    instances, ent, boxes = mixed(count, seed=count)
    if count == 0:
        instances = [[np.array([0.0, 0.0, 4.0, 0.0, 4.0, 4.0])]]       # the host call wants at least one instance
    _compare(instances, ent, boxes)


def test_operator_equals_the_python_oracle(gpu_required):
    """50 entries (ten of each family whose scaled polygons the point-by-point Python restatement can walk) against
    oracle.train_oracle.rasterize_polygons_within_box."""
    from oracle.train_oracle import rasterize_polygons_within_box
    checked = 0
    for name in ORACLE_FAMILIES:
        instances, ent, boxes = family(name, 10, seed=11)
        got = rasterize_entries_device(instances, ent, boxes, S)
        for e in range(10):
            want = rasterize_polygons_within_box(instances[int(ent[e])], boxes[e].astype(np.float64), S)
            assert np.array_equal(got[e], np.asarray(want, bool)), (name, e)
            checked += 1
    assert checked == 50


def test_operator_gives_a_zero_mask_for_an_instance_out_of_range(gpu_required):
    """The device validates the instance index: outside [0, n_inst) nothing is read and the mask is zero; its neighbours are unaffected."""
    instances, ent, boxes = family("inside", 8, seed=5)
    want = rasterize_entries(instances, ent, boxes, S)
    bad = ent.copy()
    bad[2], bad[5] = -1, len(instances)
    got = rasterize_entries_device(instances, bad, boxes, S)
    keep = np.ones(8, bool)
    keep[[2, 5]] = False
    assert not got[2].any() and not got[5].any() and np.array_equal(got[keep], want[keep])


# ---------------------------------------------------------------------------------------------------------------- the step
SPEC = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)


def _problem():
    gt_boxes = [np.array([[20.0, 30.0, 120.0, 160.0], [150.0, 40.0, 300.0, 130.0]], np.float32), np.array([[100.0, 100.0, 260.0, 280.0]], np.float32)]
    gt_classes = [np.array([0, 1]), np.array([1])]

    def blob(b, k):
        cx, cy, rx, ry = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, (b[2] - b[0]) / 2, (b[3] - b[1]) / 2
        th = np.linspace(0, 2 * np.pi, k, endpoint=False)
        return [np.stack([cx + rx * np.cos(th), cy + ry * np.sin(th)], 1).reshape(-1)]
    polys = [[blob(b, 7 + i) for i, b in enumerate(bs)] for bs in gt_boxes]
    return gt_boxes, gt_classes, polys


def _pair(precision, batch=2):
    spec = EngineSpec(**SPEC).replace(precision=precision)
    Wn = synthetic_weights(spec, seed=0)
    scale = 128.0 if precision == "fp16" else 1.0
    out = []
    try:
        for mode in ("host", "device"):
            tr = Trainer(spec, Wn, (256, 256, 3), batch=batch, loss_scale=scale, mask_targets=mode)
            out.append(tr)
            tr.set_sampling(256, 0.5, 64, 0.25)
    except Exception:
        for tr in out:
            tr.close()
        raise
    return out


def _live_targets(tr):
    total = int(tr.tensor("mask_total")[0])
    return total, tr.tensor("mask_targets")[:total]


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_step_is_bit_identical_to_host_mode(gpu_required, precision):
    """Two trainers on the same weights, batch and seed, one per mode: after one train_step the live mask targets, the five losses and
    the whole flat gradient are the same bits; after three steps with apply_sgd so are the master weights."""
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem()
    host, dev = _pair(precision)
    try:
        lh = host.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        ld = dev.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        nh, th = _live_targets(host)
        nd, td = _live_targets(dev)
        fg = dev.tensor("roi_sampled_count")[:2, 0]
        print(f"{precision}: {nd} mask entries, foreground per image {fg.tolist()}, target foreground {float(td.mean()):.3f}, losses {ld}")
        assert nh == nd and nd > 0 and int(fg.max()) > 1, "the batch must give an image more than one foreground entry"
        assert td.any() and np.array_equal(th, td)
        assert [lh[k] for k in NAMES] == [ld[k] for k in NAMES]
        assert np.array_equal(host.flat("grad"), dev.flat("grad"))
        for it in range(3):
            if it:
                host.train_step(tiles, gt_boxes, gt_classes, polys, seed=5 + it)
                dev.train_step(tiles, gt_boxes, gt_classes, polys, seed=5 + it)
            host.apply_sgd(1e-3, 0.9, 1e-4)
            dev.apply_sgd(1e-3, 0.9, 1e-4)
        assert np.array_equal(host.flat("master"), dev.flat("master"))
        assert dev.mask_target_fallbacks == 0 and host.mask_target_fallbacks == 0
        for tr in (host, dev):                                  # the stage list is built by the first set_profiling
            tr.set_profiling(True)
            tr.set_profiling(False)
        assert "mask.targets" in [s["name"] for s in dev.stage_times()] and "mask.targets" not in [s["name"] for s in host.stage_times()]
    finally:
        host.close()
        dev.close()


def test_batch_beyond_the_pool_takes_the_host_path_for_that_step(gpu_required):
    """The pool of a batch-2 trainer holds 2 * 65536 doubles: a batch with a 66 000-vertex polygon does not fit, runs on the host --
    same losses and gradient bits as host mode, one fallback counted -- and the next batch, which fits, is on the device again."""
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem()
    b = gt_boxes[1][0]
    th = np.linspace(0, 2 * np.pi, 66000, endpoint=False)
    big = [polys[0], [[np.stack([(b[0] + b[2]) / 2 + (b[2] - b[0]) / 2 * np.cos(th), (b[1] + b[3]) / 2 + (b[3] - b[1]) / 2 * np.sin(th)], 1).reshape(-1)]]]
    assert sum(p.size for img in big for inst in img for p in inst) > 2 * 65536
    host, dev = _pair("fp16")
    try:
        assert dev.set_polygons(polys) and not dev.set_polygons(big)
        lh = host.train_step(tiles, gt_boxes, gt_classes, big, seed=5)
        ld = dev.train_step(tiles, gt_boxes, gt_classes, big, seed=5)
        assert dev.mask_target_fallbacks == 1
        assert [lh[k] for k in NAMES] == [ld[k] for k in NAMES] and np.array_equal(host.flat("grad"), dev.flat("grad"))
        dev.set_profiling(True)
        lh = host.train_step(tiles, gt_boxes, gt_classes, polys, seed=6)
        ld = dev.train_step(tiles, gt_boxes, gt_classes, polys, seed=6)
        calls = {s["name"]: s["calls"] for s in dev.stage_times()}
        dev.set_profiling(False)
        assert dev.mask_target_fallbacks == 1 and calls["mask.targets"] == 1, "the batch that fits must be rasterised on the device"
        assert [lh[k] for k in NAMES] == [ld[k] for k in NAMES] and np.array_equal(host.flat("grad"), dev.flat("grad"))
    finally:
        host.close()
        dev.close()


def test_mask_backward_device_without_polygons_is_an_argument_error(gpu_required):
    """rs_trainer_mask_backward_device needs the polygons of the current targets: without rs_trainer_set_polygons since the last
    rs_trainer_set_targets it returns RS_ERR_ARG (-1) and launches nothing; the trainer then completes a host-mode step."""
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem()
    spec = EngineSpec(**SPEC)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=128.0)
    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        tr.set_targets(gt_boxes, gt_classes)
        tr.forward_trunk(tr.upload_tiles(tiles), 2)
        tr.rpn_forward(2)
        tr.roi_step(2, seed=5)
        tr.mask_forward(2)
        assert tr.lib.rs_trainer_mask_backward_device(tr._h, 2) == -1
        assert b"rs_trainer_set_polygons" in tr.lib.rs_last_error()
        assert tr.set_polygons(polys)
        tr.set_targets(gt_boxes, gt_classes)                   # new targets: the polygons on the device are the previous batch's
        assert tr.lib.rs_trainer_mask_backward_device(tr._h, 2) == -1
        losses = tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        assert all(np.isfinite(losses[k]) and losses[k] > 0 for k in NAMES)
    finally:
        tr.close()


def test_train_model_cli_writes_the_same_losses_in_both_modes(gpu_required, tmp_path):
    """train_model.py --mask-targets device against --mask-targets host on the tiny data set of the CLI test: the same total_loss and
    five losses per iteration in metrics.json."""
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    cwd = os.getcwd()
    lines = {}
    try:
        for mode in ("host", "device"):
            root = tmp_path / mode
            root.mkdir()
            wd = _tiny_training_workdir(root)
            assert train_model.main([str(root / "config.yaml"), "--synthetic-weights", "--max-iter", "3", "--log-period", "1", "--loss-scale", "256",
                                     "--precision", "fp16", "--tagged-samples", "0", "--mask-targets", mode]) == 0
            os.chdir(cwd)
            lines[mode] = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
    finally:
        os.chdir(cwd)
    assert [l["iteration"] for l in lines["host"]] == [l["iteration"] for l in lines["device"]] == [0, 1, 2]
    for h, d in zip(lines["host"], lines["device"]):
        assert all(np.isfinite(h[k]) for k in NAMES) and h["loss_mask"] > 0
        assert [h[k] for k in ("total_loss",) + NAMES] == [d[k] for k in ("total_loss",) + NAMES], (h, d)
    assert lines["host"][-1]["validation_loss"] == lines["device"][-1]["validation_loss"]
