"""Training diagnostics on the GPU (rs_trainer_set_train_stats, the three counting kernels of csrc/train_kernels.hip), exact against
the numpy reference tests/train_stats_ref.py: the operators on the cases of tests/train_stats_cases.py, the assembled step in both
trainer precisions on the tensors it read, and train_model's --train-stats.  Everything is integers, so every comparison is
np.array_equal."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from proj_roadsurf_amd import engine as E
from proj_roadsurf_amd.engine import RsError, Trainer, _check, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests import train_stats_ref as R
from tests.test_gpu_train_classes import _problem, _spec
from tests.train_stats_cases import box_cases, label_cases, mask_cases
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu

NAMES = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
BOX_KEYS = {"fast_rcnn/cls_accuracy", "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative"}
MASK_KEYS = {"mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative"}


def _dev(a, dtype):
    """Device copy of ``a`` (at least one element, so that an empty case still hands the operator a real pointer)."""
    a = np.ascontiguousarray(a, dtype)
    return torch.from_numpy(a if a.size else np.zeros(1, dtype)).to("cuda:0")


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def op_label_counts(lib, labels, out=None):
    out = torch.zeros(2, dtype=torch.int32, device="cuda:0") if out is None else out
    d = _dev(labels, np.int32)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_label_counts(_vp(d), len(labels), _vp(out), None), "rs_op_label_counts")
    torch.cuda.synchronize()
    return out


def op_box_stats(lib, c, out=None):
    out = torch.zeros(7, dtype=torch.int32, device="cuda:0") if out is None else out
    pred, cls = _dev(c["pred"], np.float32), _dev(c["cls"], np.int32)
    sc = _dev(c["sampled"], np.int32) if c["sampled"] is not None else None
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_box_stats(_vp(pred), _vp(cls), len(c["cls"]), c["K"], c["cs"], _vp(sc), 0 if sc is None else len(c["sampled"]), _vp(out), None),
           "rs_op_box_stats")
    torch.cuda.synchronize()
    return out


def op_mask_stats(lib, c, out=None):
    out = torch.zeros(5, dtype=torch.int32, device="cuda:0") if out is None else out
    lg, tg, cl = _dev(c["logits"], np.float32), _dev(c["targets"], np.uint8), _dev(c["cls"], np.int32)
    ptr = _dev([c["ptr"]], np.int32) if c["ptr"] is not None else None
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_mask_stats(_vp(lg), _vp(tg), _vp(cl), _vp(ptr), c["n_masks"], c["side"], c["cs"], _vp(out), None), "rs_op_mask_stats")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", label_cases(), ids=lambda c: c["name"])
def test_label_counts_equal_numpy(gpu_required, case):
    got = op_label_counts(load_library(), case["labels"]).cpu().numpy()
    assert np.array_equal(got, R.label_counts(case["labels"])), (got, R.label_counts(case["labels"]))


@pytest.mark.parametrize("case", box_cases(), ids=lambda c: c["name"])
def test_box_stats_equal_numpy(gpu_required, case):
    got = op_box_stats(load_library(), case).cpu().numpy()
    want = R.box_stats(case["pred"], case["cls"], case["K"], case["sampled"])
    assert np.array_equal(got, want), (case["name"], got, want)


@pytest.mark.parametrize("case", mask_cases(), ids=lambda c: c["name"])
def test_mask_stats_equal_numpy(gpu_required, case):
    got = op_mask_stats(load_library(), case).cpu().numpy()
    want = R.mask_stats(case["logits"], case["targets"], case["cls"], case["ptr"])
    assert np.array_equal(got, want), (case["name"], got, want)


def test_two_launches_into_one_table_add(gpu_required):
    lib = load_library()
    b, m, l = box_cases()[6], mask_cases()[3], label_cases()[4]["labels"]
    for fn, case, want in ((op_box_stats, b, R.box_stats(b["pred"], b["cls"], b["K"], b["sampled"])),
                           (op_mask_stats, m, R.mask_stats(m["logits"], m["targets"], m["cls"], m["ptr"])),
                           (op_label_counts, l, R.label_counts(l))):
        out = fn(lib, case)
        assert want.any()
        assert np.array_equal(fn(lib, case, out=out).cpu().numpy(), 2 * want)


# ------------------------------------------------------------------ the assembled step

def _reference_table(tr, n=2):
    """The table from the tensors the three stages read, copied back after the step."""
    K = tr.spec.num_classes
    kw = {}
    if tr.spec.mask_on:
        lg = tr.tensor("t:mask_logits")
        kw = dict(mask_logits=lg, mask_targets=tr.tensor("mask_targets").reshape(lg.shape[0], -1), mask_classes=tr.tensor("mask_classes"),
                  mask_total=int(tr.tensor("mask_total")[0]))
    return R.table(tr.tensor("rpn_labels")[:n], tr.tensor("roi_classes")[:n], tr.tensor("roi_sampled_count")[:n],
                   tr.tensor("box_pred", engine=True).reshape(-1, 1024, (5 * K + 1 + 15) // 16 * 16)[:n], K, **kw)


def _stage_names(tr):
    tr.set_profiling(False)
    return [s["name"] for s in tr.stage_times()]


@pytest.fixture(scope="module", params=[(3, "fp32"), (8, "fp16")], ids=lambda p: f"K{p[0]}-{p[1]}")
def step(request, gpu_required):
    """One trainer of the small configuration (256 x 256 tiles, batch 2, 300 proposals, sampling 256 / 128) and the same batch and seed
    run with the switch off, on, on again, and on with the mask targets rasterised on the device; everything the tests read is copied
    to the host."""
    K, precision = request.param
    spec = _spec(K, precision)
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem(K)
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=1.0 if precision == "fp32" else 128.0)
    try:
        tr.set_sampling(256, 0.5, 128, 0.25)
        out = dict(K=K, precision=precision)
        out["stages_off"], out["tensors_off"] = _stage_names(tr), tr.tensor_names()
        with pytest.raises(RsError):
            tr.tensor("train_stats")                       # not allocated before the first switch-on
        out["losses_off"] = tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        out["grad_off"] = tr.flat("grad").copy()
        tr.set_train_stats(True)
        out["losses_on"] = tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        out["grad_on"] = tr.flat("grad").copy()
        out["table"] = tr.train_stats_table().copy()
        out["scalars"] = tr.train_stats()
        out["want"] = _reference_table(tr)
        out["mask_total"] = int(tr.tensor("mask_total")[0])
        out["stages_on"], out["tensors_on"] = _stage_names(tr), tr.tensor_names()
        tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        out["table_again"] = tr.train_stats_table().copy()
        tr.mask_targets = "device"
        tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        assert tr.mask_target_fallbacks == 0
        out["table_device"] = tr.train_stats_table().copy()
        tr.mask_targets = "host"
        # both images without ground truth: the form tests/test_gpu_trainer.py trains on
        none_b, none_c = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
        tr.train_step(tiles, [none_b, none_b], [none_c, none_c], [[], []], seed=4)
        out["table_empty"], out["scalars_empty"], out["want_empty"] = tr.train_stats_table().copy(), tr.train_stats(), _reference_table(tr)
        tr.set_train_stats(False)
        with pytest.raises(RsError):
            tr.train_stats()
        yield out
    finally:
        tr.close()


def test_step_table_equals_numpy_on_the_tensors_read_back(step):
    print(f"K={step['K']} {step['precision']}: table {step['table'].tolist()} scalars {step['scalars']}")
    assert step["table"].dtype == np.int32 and step["table"].shape == (16,)
    assert np.array_equal(step["table"], step["want"]), (step["table"].tolist(), step["want"].tolist())
    assert step["scalars"] == E.train_stats_scalars(step["want"]) and set(step["scalars"]) == set(E.TRAIN_STATS_KEYS)


def test_step_table_invariants(step):
    pos, neg, fg, bg, inst, correct, fgn, fg_correct, fg_as_bg, pixels, incorrect, positive, false_pos, false_neg, n, last = step["table"].tolist()
    assert n == 2 and last == 0
    assert inst == fg + bg and fgn == fg and fg > 0 and bg > 0
    assert pixels == step["mask_total"] * 784 and step["mask_total"] == fg
    assert incorrect == false_pos + false_neg and 0 < positive < pixels
    assert 0 < pos and pos + neg <= 2 * 256 and fg + bg <= 2 * 128
    assert fg_correct + fg_as_bg <= fgn and correct <= inst


def test_switch_leaves_losses_and_gradients_bit_for_bit(step):
    assert [step["losses_on"][k] for k in NAMES] == [step["losses_off"][k] for k in NAMES]
    assert tuple(step["losses_on"]) == NAMES                                  # train_step keeps returning exactly the five losses
    assert step["grad_off"].any() and np.array_equal(step["grad_on"], step["grad_off"])


def test_two_runs_and_both_mask_target_modes_give_the_same_table(step):
    assert np.array_equal(step["table_again"], step["table"])
    assert np.array_equal(step["table_device"], step["table"])


def test_batch_without_ground_truth_reports_accuracy_only(step):
    t, s = step["table_empty"], step["scalars_empty"]
    assert np.array_equal(t, step["want_empty"])
    assert t[0] == 0 and t[2] == 0 and t[6] == 0 and not t[9:14].any() and t[4] == t[3] > 0
    assert "fast_rcnn/cls_accuracy" in s and not (set(s) & (BOX_KEYS - {"fast_rcnn/cls_accuracy"})) and not (set(s) & MASK_KEYS)
    assert s["rpn/num_pos_anchors"] == 0.0 and s["roi_head/num_fg_samples"] == 0.0


def test_default_trainer_keeps_its_stages_and_tensors(step):
    """Never switched on: no stats stage, no stats tensor.  Switched on: the three stages are appended last, the enumerated tensor
    table is the same (the table is read by name only)."""
    assert not [s for s in step["stages_off"] if s.endswith(".stats")] and "train_stats" not in step["tensors_off"]
    assert step["stages_on"] == step["stages_off"] + ["box.stats", "mask.stats", "rpn.stats"]
    assert step["tensors_on"] == step["tensors_off"]


def test_mask_off_trainer_gives_no_mask_keys(gpu_required):
    spec = _spec(3, "fp16").replace(mask_on=False)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=128.0, train_stats=True)
    try:
        tr.set_sampling(256, 0.5, 128, 0.25)
        gt_boxes, gt_classes, polys = _problem(3)
        tr.train_step(synthetic_tiles(2, 256, 256, 3, seed=777), gt_boxes, gt_classes, polys, seed=5)
        t, s = tr.train_stats_table(), tr.train_stats()
        assert np.array_equal(t, _reference_table(tr))
        assert not t[9:14].any() and set(s) == set(E.TRAIN_STATS_KEYS) - MASK_KEYS
        assert _stage_names(tr)[-2:] == ["box.stats", "rpn.stats"]
    finally:
        tr.close()


def test_switch_refuses_other_values(gpu_required):
    spec = _spec(3, "fp16")
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=128.0)
    try:
        assert tr.lib.rs_trainer_set_train_stats(tr._h, 2) != 0 and b"rs_trainer_set_train_stats" in tr.lib.rs_last_error()
        assert tr.lib.rs_trainer_set_train_stats(tr._h, 1) == 0 and tr.lib.rs_trainer_set_train_stats(tr._h, 0) == 0
    finally:
        tr.close()


# ------------------------------------------------------------------ the command line

def _run_cli(tmp_path, name, eval_period, extra):
    """train_model on the tiny training set of tests/test_gpu_trainer.py: three iterations, every one logged."""
    import yaml
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    root = tmp_path / name
    root.mkdir()
    wd = _tiny_training_workdir(root)
    d2 = yaml.safe_load(open(root / "d2.yaml"))
    d2["TEST"]["EVAL_PERIOD"] = eval_period
    yaml.safe_dump(d2, open(root / "d2.yaml", "w"))
    cwd = os.getcwd()
    try:
        assert train_model.main([str(root / "config.yaml"), "--synthetic-weights", "--log-period", "1", "--loss-scale", "256", "--precision", "fp16",
                                 "--max-iter", "3", "--tagged-samples", "0", "--val-max-images", "2"] + extra) == 0
    finally:
        os.chdir(cwd)
    return [json.loads(l) for l in open(wd / "logs" / "metrics.json")]


@pytest.fixture(scope="module")
def cli(gpu_required, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("train_stats_cli")
    return dict(on=_run_cli(tmp, "on", 3, ["--train-stats"]), on_noval=_run_cli(tmp, "on_noval", 0, ["--train-stats"]), off=_run_cli(tmp, "off", 3, []))


def test_cli_records_carry_the_ten_keys_in_range(cli):
    assert [r["iteration"] for r in cli["on"]] == [0, 1, 2]
    for r in cli["on"]:
        print({k: r[k] for k in E.TRAIN_STATS_KEYS})
        assert set(E.TRAIN_STATS_KEYS) <= set(r)
        assert all(0.0 <= r[k] <= 1.0 for k in BOX_KEYS | MASK_KEYS)
        assert 0 < r["rpn/num_pos_anchors"] and r["rpn/num_pos_anchors"] + r["rpn/num_neg_anchors"] <= 64
        assert 0 < r["roi_head/num_fg_samples"] and r["roi_head/num_fg_samples"] + r["roi_head/num_bg_samples"] <= 64     # ROI_HEADS.BATCH_SIZE_PER_IMAGE


def test_cli_validation_iterations_carry_the_training_steps_table(cli):
    """Iteration 2 runs the validation pass (train_step on the same trainer) before its record is written; the run without validation
    shows what the training step counted."""
    assert ["validation_loss" in r for r in cli["on"]] == [False, False, True] and not any("validation_loss" in r for r in cli["on_noval"])
    for a, b in zip(cli["on"], cli["on_noval"]):
        assert {k: a[k] for k in E.TRAIN_STATS_KEYS} == {k: b[k] for k in E.TRAIN_STATS_KEYS}
        assert [a[k] for k in NAMES] == [b[k] for k in NAMES]


def test_cli_without_the_switch_is_the_parents_record(cli):
    for a, b in zip(cli["on"], cli["off"]):
        assert not (set(b) & set(E.TRAIN_STATS_KEYS))
        assert set(a) - set(E.TRAIN_STATS_KEYS) == set(b)
        assert [a[k] for k in NAMES] == [b[k] for k in NAMES]
