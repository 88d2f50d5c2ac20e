"""torchvision's batched_nms size rule (EngineSpec.batched_nms = "torchvision") on the GPU: the operator on fixtures that tell
the rule's arithmetic from per-category arithmetic, then both NMS stages of the inference engine, the trainer's proposal stage
and the CLI, each against the oracle on the engine's OWN stage inputs.  The reference is tests/batched_nms_ref.py rule_keep,
which tests/test_batched_nms_cpu.py holds equal to oracle.batched_nms."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd.engine import Engine, LanePipeline, Predictor, Trainer, _check, load_library, make_rs_spec
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests import batched_nms_ref as R
from tests.test_gpu_engine import _rpn_inputs, _strict_compare
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from oracle import maskrcnn_oracle as O
    return O


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ operator
# name: (category slots per image, capacity, images).  Segments = images x slots: <= 32 take the global-memory mask (mask build shared
# by several workgroups + scan launch), more the LDS mask; capacity 2048 always the global-memory mask.
OPERATOR_CALLS = {
    "lds_8_slots": (8, 1024, [("pairs", [0, 1]), ("pairs", [0, 2, 3, 5, 7]), ("pairs", list(range(8))), ("total", 1000, [1, 4]),
                              ("total", 1001, [1, 4]), ("empty",), ("single",), ("invalid", 1100, 150, [2, 6]),
                              ("total", 1000, list(range(8))), ("total", 1001, list(range(8)))]),
    "global_2_slots": (2, 1024, [("pairs", [0, 1]), ("total", 1000, [0, 1]), ("total", 1001, [0, 1]), ("invalid", 1100, 150, [0, 1])]),
    "global_5_slots": (5, 1024, [("pairs", list(range(5))), ("total", 1001, list(range(5))), ("single",), ("total", 1000, [0, 3, 4])]),
    "cap2048_5_slots": (5, 2048, [("pairs", list(range(5))), ("total", 1001, list(range(5))), ("invalid", 2500, 1500, [1, 3]),
                                  ("empty",), ("total", 1000, [0, 4])]),
}


def _run_op(lib, boxes, valid, counts, thresh, rule):
    """rule 0 / 1: rs_op_batched_nms; None: rs_op_nms over all segments."""
    I, G, cap = valid.shape
    bd, cd, vd = _dev(boxes), _dev(counts), _dev(valid)
    keep = torch.full((I, G, cap), 7, dtype=torch.uint8, device=bd.device)
    torch.cuda.synchronize()
    if rule is None:
        _check(lib, lib.rs_op_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), I * G, cap, thresh, None), "rs_op_nms")
    else:
        _check(lib, lib.rs_op_batched_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), I, G, cap, thresh, rule, None), "rs_op_batched_nms")
    torch.cuda.synchronize()
    return keep.cpu().numpy()


def _run_op_decision(lib, boxes, valid, counts, thresh):
    """rs_op_batched_nms_decision, rule = 1: keep flags and what the NMS kernel itself decided per image."""
    I, G, cap = valid.shape
    bd, cd, vd = _dev(boxes), _dev(counts), _dev(valid)
    keep = torch.full((I, G, cap), 7, dtype=torch.uint8, device=bd.device)
    rule = torch.full((I, 2), -7, dtype=torch.int32, device=bd.device)
    unit = torch.full((I,), -7.0, dtype=torch.float32, device=bd.device)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_batched_nms_decision(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), I, G, cap, thresh, 1, _ptr(rule), _ptr(unit), None),
           "rs_op_batched_nms_decision")
    torch.cuda.synchronize()
    return keep.cpu().numpy(), rule.cpu().numpy(), unit.cpu().numpy()


@pytest.mark.parametrize("t", [0.5, 0.7])
@pytest.mark.parametrize("call", list(OPERATOR_CALLS))
def test_batched_nms_operator_follows_the_size_rule(gpu_required, call, t):
    """rs_op_batched_nms(rule = 1) == the rule's reference exactly, image by image: images of 2, 5 and 8 categories, totals of
    1000 (rule taken), 1001 (not taken), 0 and 1 boxes, raw counts above 1000 that invalid entries bring down to 950 / 1000
    (taken), near-threshold pairs + the pair classes of tests/util.py nms_edge_pairs, thresholds as make_rs_spec writes them, in
    every form of the NMS kernel.  Before the GPU is asked, the oracle confirms that the fixture discriminates: in every image
    that takes the rule and has two or more populated categories the two branches of oracle.batched_nms differ in >= 8 keep
    flags, so per-category arithmetic cannot pass.  Images that do not take the rule equal rs_op_nms; rule = 0 equals rs_op_nms
    bit for bit everywhere."""
    lib = load_library()
    G, cap, kinds = OPERATOR_CALLS[call]
    thresh = make_rs_spec(EngineSpec(nms_thresh_test=t)).nms_thresh_test
    assert thresh == make_rs_spec(EngineSpec(rpn_nms_thresh=t)).rpn_nms_thresh
    boxes, valid, counts = R.operator_fixture(G, cap, t, seed=len(call) * 100 + int(t * 10), kinds=kinds)
    I = len(kinds)
    assert (I * G > 32) == call.startswith("lds")
    want = np.zeros(valid.shape, bool)
    taken, units, totals = [], [], []
    for i in range(I):
        want[i], tk, un, tot = R.rule_keep(boxes[i], valid[i], counts[i], t)
        taken.append(tk); units.append(un); totals.append(tot)
        assert np.array_equal(want[i], R.oracle_keep(boxes[i], valid[i], counts[i], t, coordinate_trick=None)), (call, i)
        if tk and int((counts[i] > 0).sum()) >= 2:
            plain = R.oracle_keep(boxes[i], valid[i], counts[i], t, coordinate_trick=False)
            differ = int((plain != R.oracle_keep(boxes[i], valid[i], counts[i], t, coordinate_trick=True)).sum())
            print(f"batched_nms fixture {call} t={t} image {i} ({kinds[i][0]}): total {tot}, branches differ in {differ} flags")
            assert differ >= 8, (call, t, i, kinds[i], differ)
    # the fixture holds what its kinds say
    for i, kind in enumerate(kinds):
        if kind[0] == "total":
            assert totals[i] == kind[1] and taken[i] == (kind[1] <= 1000)
        elif kind[0] == "invalid":
            assert int(counts[i].sum()) == kind[1] > 1000 and totals[i] == kind[1] - kind[2] <= 1000 and taken[i]
        elif kind[0] == "empty":
            assert totals[i] == 0 and not taken[i]
        elif kind[0] == "single":
            assert totals[i] == 1 and taken[i]
        else:
            assert taken[i] and int((counts[i] > 0).sum()) == len(kind[1])
    assert any(taken) and not all(taken)

    got, rule, unit = _run_op_decision(lib, boxes, valid, counts, thresh)
    assert rule[:, 0].tolist() == [int(x) for x in taken] and rule[:, 1].tolist() == totals
    assert np.array_equal(unit, np.array(units, np.float32)), (unit, units)
    assert np.array_equal(got, _run_op(lib, boxes, valid, counts, thresh, 1))
    plain = _run_op(lib, boxes, valid, counts, thresh, None)
    assert set(np.unique(got).tolist()) <= {0, 1}
    for i in range(I):
        for g in range(G):
            c = int(counts[i, g])
            assert np.array_equal(got[i, g, :c].astype(bool), want[i, g, :c]), \
                (call, t, i, g, kinds[i], np.nonzero(got[i, g, :c].astype(bool) != want[i, g, :c])[0][:8])
            assert (got[i, g, c:] == 0).all()
        if not taken[i]:
            assert np.array_equal(got[i], plain[i]), (call, i)
    assert np.array_equal(_run_op(lib, boxes, valid, counts, thresh, 0), plain)
    # and the per-category kernel does differ from the rule where the oracle says so (the discrimination is real on the device too)
    assert any(not np.array_equal(plain[i].astype(bool), want[i]) for i in range(I) if taken[i])


def test_batched_nms_operator_rejects_bad_arguments(gpu_required):
    lib = load_library()
    b, v, c = R.operator_fixture(2, 1024, 0.5, 3, [("single",)])
    bd, cd, vd = _dev(b), _dev(c), _dev(v)
    keep = torch.zeros(v.shape, dtype=torch.uint8, device=bd.device)
    assert lib.rs_op_batched_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), 1, 2, 1024, 0.5, 2, None) < 0
    assert lib.rs_op_batched_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), 1, 0, 1024, 0.5, 1, None) < 0
    assert lib.rs_op_batched_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), 1, 2, 4096, 0.5, 1, None) < 0
    # entries beyond the capacity are counted but hold no box: the rule is only offered where 1000 boxes fit a segment
    assert lib.rs_op_batched_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), 1, 2, 1000, 0.5, 1, None) < 0
    assert b"1000" in lib.rs_last_error()
    rule = torch.zeros((1, 2), dtype=torch.int32, device=bd.device)
    assert lib.rs_op_batched_nms_decision(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), 1, 2, 1024, 0.5, 0, _ptr(rule), None, None) < 0


# ------------------------------------------------------------------ engine: RPN
BRANCH_DIFFS = {}        # (test, what) -> (image, segment) pairs on which the two oracle branches differ; printed for DESIGN.md section 4


def _count_branch_diffs(key, boxes, valid, counts, t):
    a = R.category_keep(boxes, valid, counts, t)
    b = R.category_keep(boxes, valid, counts, t, R.rule_decision(boxes, valid, counts)[1])
    d = int(sum(not np.array_equal(a[g], b[g]) for g in range(len(counts))))
    BRANCH_DIFFS[key] = BRANCH_DIFFS.get(key, 0) + d
    return d


def check_rpn_rule(spec, eng, n, key, expect_taken):
    """rpn_cand_keep == the rule's reference from rpn_cand_boxes / rpn_cand_valid / rpn_cand_count, rpn_nms_rule / rpn_nms_unit ==
    its decision, and O.rpn_proposals(nms_trick=None) on the engine's own head outputs == the engine's proposals (bounds of
    tests/test_gpu_engine.py check_rpn_stage).  Returns the valid totals per image."""
    O = _oracle()
    cb, cv = eng.tensor("rpn_cand_boxes", n=n), eng.tensor("rpn_cand_valid", n=n)
    ck, cc = eng.tensor("rpn_cand_keep", n=n), eng.tensor("rpn_cand_count", n=n)
    rule, unit = eng.tensor("rpn_nms_rule", n=n), eng.tensor("rpn_nms_unit", n=n)
    totals = []
    for i in range(n):
        want, taken, un, total = R.rule_keep(cb[i], cv[i], cc[i], spec.rpn_nms_thresh)
        totals.append(total)
        assert taken == expect_taken, (i, total)
        assert (int(rule[i, 0]), int(rule[i, 1])) == (int(taken), total) and float(unit[i]) == float(un), (i, rule[i], unit[i], un)
        for l in range(cc.shape[1]):
            c = int(cc[i, l])
            assert np.array_equal(ck[i, l, :c].astype(bool), want[l, :c]), f"image {i} level {l}: RPN NMS keep flags differ from the rule's"
        if taken:
            _count_branch_diffs(key, cb[i], cv[i], cc[i], spec.rpn_nms_thresh)
    logits, deltas = _rpn_inputs(spec, eng, n)
    nh, nw, _, _ = eng.net_shape()
    ref = O.rpn_proposals(spec, logits, deltas, [(nh, nw)] * n, nms_trick=None)
    pb, pl, pc = eng.tensor("proposal_boxes", n=n), eng.tensor("proposal_logits", n=n), eng.tensor("proposal_count", n=n)
    for i in range(n):
        m = int(pc[i])
        assert m == ref[i]["boxes"].shape[0], f"image {i}: {m} proposals vs {ref[i]['boxes'].shape[0]}"
        assert ref[i]["pre_nms"]["boxes_clipped"].shape[0] == totals[i]
        assert np.array_equal(pl[i, :m], ref[i]["logits"].numpy())
        assert np.abs(pb[i, :m] - ref[i]["boxes"].numpy()).max() <= 1e-3
    return totals


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_rpn_nms_follows_the_size_rule(gpu_required, precision):
    """PRE_NMS_TOPK_TEST 150 x 5 levels <= 1000 candidates: every image takes the rule -- batch 4 eagerly, single tiles eagerly, at
    graph capture and at replay, and on both lanes of a LanePipeline.  The same spec with the default PRE_NMS_TOPK_TEST has more than
    1000 valid candidates per image and equals the per-category reference: the rule decides, not the mode."""
    spec = EngineSpec(num_classes=2, precision=precision, rpn_pre_nms_topk_test=150, batched_nms="torchvision")
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(8, 512, 512, 3, seed=4711)
    key = f"rpn/{precision}"
    eng = Engine(spec, W, (512, 512, 3), max_batch=4)
    try:
        names = [s["name"] for s in eng.stage_times()]
        assert not [n for n in names if "nms_rule" in n]          # the rule is decided inside rpn.nms / box.nms: no launch of its own
        eng.infer(tiles[:4])
        totals = check_rpn_rule(spec, eng, 4, key, True)
        assert max(totals) <= 1000 and min(totals) >= 1, totals
        for k in range(4):                       # one tile per call: eager, graph capture, replay, replay
            eng.infer(tiles[4 + k:5 + k])
            check_rpn_rule(spec, eng, 1, key, True)
    finally:
        eng.close()
    pipe = LanePipeline(spec, W, (512, 512, 3), max_batch=4, lanes=2)
    try:
        for k in range(2):
            lane = pipe.lane_of_next()
            idx = pipe.submit(lane.upload_tiles(tiles[4 * k:4 * k + 4]), 4)
            assert idx == k
        pipe.flush()
        for k in range(2):
            pipe.engines[k].fetch(4)
            check_rpn_rule(spec, pipe.engines[k], 4, key, True)
    finally:
        pipe.close()
    big = spec.replace(rpn_pre_nms_topk_test=EngineSpec().rpn_pre_nms_topk_test)
    eng = Engine(big, W, (512, 512, 3), max_batch=4)
    try:
        eng.infer(tiles[:4])
        totals = check_rpn_rule(big, eng, 4, key + "/default_topk", False)
        assert min(totals) > 1000, totals
    finally:
        eng.close()
    print("batched_nms branch differences (image, level) pairs:", {k: v for k, v in BRANCH_DIFFS.items() if k.startswith(key)})


# ------------------------------------------------------------------ engine: box head
def check_box_rule(spec, eng, dets, n, tile_hw, key, expect_taken):
    """box_seg_keep == the rule's reference per image from box_seg_boxes / box_seg_count; fast_rcnn_inference_single_image(nms_trick=None)
    + detector_postprocess on the engine's own box-head output reproduce count, classes and order exactly, scores and boxes within
    the bounds of tests/test_gpu_engine.py check_box_postprocess."""
    O = _oracle()
    K = spec.num_classes
    sb, sk, sc = eng.tensor("box_seg_boxes", n=n), eng.tensor("box_seg_keep", n=n), eng.tensor("box_seg_count", n=n)
    rule, unit = eng.tensor("box_nms_rule", n=n), eng.tensor("box_nms_unit", n=n)
    totals = []
    for i in range(n):
        want, taken, un, total = R.rule_keep(sb[i], None, sc[i], spec.nms_thresh_test)
        totals.append(total)
        assert taken == expect_taken, (i, total)
        assert (int(rule[i, 0]), int(rule[i, 1])) == (int(taken), total) and float(unit[i]) == float(un)
        for k in range(K):
            c = int(sc[i, k])
            assert np.array_equal(sk[i, k, :c].astype(bool), want[k, :c]), f"image {i} class {k}: box NMS keep flags differ from the rule's"
        if taken:
            _count_branch_diffs(key, sb[i], None, sc[i], spec.nms_thresh_test)
    nh, nw, _, _ = eng.net_shape()
    pred = torch.from_numpy(eng.tensor("box_pred", n=n))
    pb = torch.from_numpy(eng.tensor("proposal_boxes", n=n))
    pc = eng.tensor("proposal_count", n=n)
    dn = eng.tensor("det_boxes_net", n=n)
    for i in range(n):
        m = int(pc[i])
        probs = F.softmax(pred[i, :m, :K + 1], dim=-1)
        dec = O.apply_deltas(pred[i, :m, K + 1:5 * K + 1], pb[i, :m], spec.box_reg_weights, spec.scale_clamp)
        ref = O.fast_rcnn_inference_single_image(spec, dec, probs, (nh, nw), nms_trick=None)
        fin = O.detector_postprocess(ref, (nh, nw), tile_hw[0], tile_hw[1])
        d = dets[i]
        assert len(d) == fin["boxes"].shape[0], f"image {i}: {len(d)} detections vs {fin['boxes'].shape[0]}"
        assert np.array_equal(d.pred_classes, fin["classes"].numpy())
        if len(d):
            assert np.abs(d.scores - fin["scores"].numpy()).max() <= 2e-6
            assert np.abs(d.pred_boxes - fin["boxes"].numpy()).max() <= 1e-3
            assert np.abs(dn[i, :len(d)] - ref["boxes"].numpy()[: len(d)]).max() <= 2e-3
    return totals


def test_box_nms_follows_the_size_rule(gpu_required):
    """Two batches with one weight set: 300 proposals x 2 classes stay at or below 1000 candidates (rule taken, every image), 1000
    proposals x 2 classes at the default spec exceed it (per-category, every image); both are asserted to occur."""
    small = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                       batched_nms="torchvision")
    W = synthetic_weights(small, seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    eng = Engine(small, W, (256, 256, 3), max_batch=4)
    try:
        dets = eng.infer(tiles, want_probs=True)
        totals = check_box_rule(small, eng, dets, 3, (256, 256), "box/fp16", True)
        assert 1 <= min(totals) and max(totals) <= 1000, totals
        assert sum(len(d) for d in dets) > 0
    finally:
        eng.close()
    big = EngineSpec(num_classes=2, batched_nms="torchvision")
    tiles = synthetic_tiles(2, 512, 512, 3, seed=1234)
    eng = Engine(big, W, (512, 512, 3), max_batch=2)
    try:
        dets = eng.infer(tiles)
        totals = check_box_rule(big, eng, dets, 2, (512, 512), "box/fp16/1000_proposals", False)
        assert min(totals) > 1000, totals
    finally:
        eng.close()
    print("batched_nms branch differences (image, class) pairs:", {k: v for k, v in BRANCH_DIFFS.items() if k.startswith("box")})


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_end_to_end_small_against_the_oracle_with_the_size_rule(gpu_required, precision):
    """OracleModel(nms_trick=None) against the engine in the new mode on the `small` configuration, within the bounds of
    tests/test_gpu_engine.py test_fp32_mode_end_to_end_small (>= 98 % matched both ways, |dscore| <= 1e-4, |dbox| <= 1e-2 px)."""
    O = _oracle()
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                      precision=precision, batched_nms="torchvision")
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    eng = Engine(spec, W, (256, 256, 3), max_batch=3)
    try:
        dets = eng.infer(tiles)
        # 300 + 300 + 300 + 108 + 27 RPN candidates per image: the box head takes the rule (<= 600 candidates), the RPN only where
        # more than 35 candidates are invalid -- the oracle follows the same rule
        rr, br = eng.tensor("rpn_nms_rule", n=3), eng.tensor("box_nms_rule", n=3)
        assert br[:, 0].all() and (br[:, 1] <= 1000).all() and np.array_equal(rr[:, 0] != 0, (rr[:, 1] >= 1) & (rr[:, 1] <= 1000))
        ref = O.OracleModel(spec, W, nms_trick=None)([tiles[i] for i in range(3)])
        for i in range(3):
            _strict_compare(ref[i], dets[i], f"batched_nms_small_{precision}[{i}]")
    finally:
        eng.close()


# ------------------------------------------------------------------ default mode untouched
def test_default_mode_is_untouched(gpu_required):
    """batched_nms="per_category" given explicitly == the argument left out: same stage list, bit-identical detections and masks;
    the stage list is the parent commit's (tests/golden/stage_names_small.json) -- in the new mode too, which only adds its four
    inspection tensors."""
    base = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)
    W = synthetic_weights(EngineSpec(**base), seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    out, names, tensors = {}, {}, {}
    for tag, spec in (("absent", EngineSpec(**base)), ("explicit", EngineSpec(batched_nms="per_category", **base)),
                      ("torchvision", EngineSpec(batched_nms="torchvision", **base))):
        eng = Engine(spec, W, (256, 256, 3), max_batch=4)
        try:
            out[tag] = eng.infer(tiles, want_probs=True)
            names[tag] = [s["name"] for s in eng.stage_times()]
            tensors[tag] = eng.tensor_names()
        finally:
            eng.close()
    assert names["absent"] == names["explicit"] and tensors["absent"] == tensors["explicit"]
    assert not [n for n in names["absent"] if "nms_rule" in n] and not [n for n in tensors["absent"] if "nms_rule" in n or "nms_unit" in n]
    with open(os.path.join(ROOT, "tests", "golden", "stage_names_small.json")) as f:
        assert names["absent"] == json.load(f), "the default engine's stage list changed"
    assert names["torchvision"] == names["absent"]                 # the rule is decided inside rpn.nms / box.nms
    assert sorted(set(tensors["torchvision"]) - set(tensors["absent"])) == ["box_nms_rule", "box_nms_unit", "rpn_nms_rule", "rpn_nms_unit"]
    for a, b in zip(out["absent"], out["explicit"]):
        assert len(a) == len(b) and len(a) > 0
        assert np.array_equal(a.pred_boxes, b.pred_boxes) and np.array_equal(a.scores, b.scores)
        assert np.array_equal(a.pred_classes, b.pred_classes) and np.array_equal(a._packed, b._packed)
        assert np.array_equal(a.mask_probs, b.mask_probs)


# ------------------------------------------------------------------ trainer
def test_training_mode_proposals_follow_the_size_rule(gpu_required):
    """rs_trainer_set_rpn_topk(150, 1000) in the new mode: 5 x 150 candidates per image take the rule in the 2048-capacity kernels, and the
    training proposals equal O.rpn_proposals(train_spec, ..., nms_trick=None) on the engine's own head outputs (shape of
    tests/test_gpu_trainer.py test_training_mode_proposals_match_oracle)."""
    O = _oracle()
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                      batched_nms="torchvision")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=888)
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=64.0)
    try:
        gt_boxes = [np.array([[20.0, 30.0, 120.0, 160.0]], np.float32), np.array([[100.0, 100.0, 260.0, 280.0], [10.0, 10.0, 60.0, 50.0]], np.float32)]
        tr.set_targets(gt_boxes, [np.array([0]), np.array([1, 1])])
        tr.set_sampling(256, 0.5, 128, 0.25)
        tr.set_rpn_topk(150, 1000)
        tr.forward_trunk(tr.upload_tiles(tiles), 2)
        tr.rpn_forward(2)
        tr.roi_step(2, seed=1)
        tr.sync()
        cand, cc = tr.tensor("roi_candidates"), tr.tensor("roi_candidate_count")
        rule, unit = tr.tensor("train_rpn_nms_rule"), tr.tensor("train_rpn_nms_unit")
        A = spec.num_anchors
        logits, deltas = [], []
        for l in range(2, 7):
            h = torch.from_numpy(tr.tensor(f"rpn_head{l}", engine=True))
            logits.append(h[..., :A].permute(0, 3, 1, 2).contiguous())
            deltas.append(h[..., A:5 * A].permute(0, 3, 1, 2).contiguous())
        train_spec = spec.replace(rpn_pre_nms_topk_test=150, rpn_post_nms_topk_test=1000)
        props = O.rpn_proposals(train_spec, logits, deltas, [(320, 320)] * 2, nms_trick=None)
        for i in range(2):
            valid_boxes = props[i]["pre_nms"]["boxes_clipped"]
            assert 1 <= valid_boxes.shape[0] <= 1000
            assert (int(rule[i, 0]), int(rule[i, 1])) == (1, valid_boxes.shape[0])
            assert float(unit[i]) == float(np.float32(np.float32(valid_boxes.max().item()) + np.float32(1)))
            pb = props[i]["boxes"].numpy()
            k = pb.shape[0]
            assert k > 0 and int(cc[i]) == k + gt_boxes[i].shape[0]
            assert float(np.abs(cand[i, :k] - pb).max()) <= 1e-3
            assert np.array_equal(cand[i, k:k + gt_boxes[i].shape[0]], gt_boxes[i])
    finally:
        tr.close()


# ------------------------------------------------------------------ CLI
def test_make_detections_cli_in_the_new_mode(gpu_required, tmp_path):
    """make_detections --batched-nms torchvision on the synthetic dataset runs, logs the mode and writes the GeoPackage; its rows equal
    the features of a Predictor built from the same YAML with batched_nms="torchvision" on the same tiles."""
    import yaml
    from proj_roadsurf_amd.gpkg import read_gpkg
    from proj_roadsurf_amd.make_detections import read_tile
    from proj_roadsurf_amd.spec import load_d2_yaml
    from proj_roadsurf_amd.vectorize import instances_to_features
    from tests.test_vector_cli import _cli_dataset
    cfg, wd = _cli_dataset(tmp_path, 6)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "proj_roadsurf_amd.make_detections", cfg, "--synthetic-weights", "--batch", "4", "--tagged-samples", "0",
                        "--batched-nms", "torchvision"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr.count("batched_nms: torchvision") == 1, r.stderr[-3000:]
    name = "val_detections_at_0dot05_threshold"
    feats = read_gpkg(str(wd / f"{name}.gpkg"), name)
    assert len(feats) > 0
    section = yaml.safe_load(open(cfg))["make_detections.py"]
    spec = load_d2_yaml(section["detectron2_config_file"], num_classes=2).replace(score_thresh_test=0.05, batched_nms="torchvision")
    pred = Predictor(spec, synthetic_weights(spec, seed=0), max_batch=4, lanes=2, on_saturation="ignore")
    try:
        files = [im["file_name"] for im in json.load(open(wd / "COCO_val.json"))["images"]]
        out = pred.predict_batch([read_tile(str(wd / f)) for f in files])
        meta = json.load(open(wd / "img_metadata.json"))
        want = []
        for f, o in zip(files, out):
            want += instances_to_features(o["instances"], os.path.basename(f), meta[f]["extent"], True, 0.75)
    finally:
        pred.close()
    assert len(want) == len(feats)
    for a, b in zip(feats, want):
        assert a["properties"]["image"] == b["properties"]["image"] and a["properties"]["det_class"] == b["properties"]["det_class"]
        assert a["properties"]["score"] == pytest.approx(b["properties"]["score"], abs=1e-7)
        assert a["geometry"]["coordinates"] == b["geometry"]["coordinates"]
