"""The trainer at every class count it accepts.  NUM_CLASSES sets the width of the fused box predictor (5K+1 rows inside
round16(5K+1): 16 rows for K <= 3 -- K = 3 fills them --, 32 for K = 4..6, 48 for K = 7, 8), the rows of the 16-row mask predictor that
are real, the columns the loss kernels read and write and the background label; the other training tests run at K = 2 only.

One assembled training step per K in {1, 3, 4, 8} in the reference-precision trainer (strict enough to pin logic) and one at K = 8 in
the fp16 trainer, against torch autograd of the oracle on the engine's own samples -- the small configuration of
tests/test_gpu_trainer.py (256x256x3 tiles resized to 320, batch 2, 300 proposals), at the bounds that file holds at K = 2 -- plus the
exact structure a class count implies (padding rows, rows of classes without a sampled foreground RoI), two optimiser steps at K = 8,
and the refusal of ground-truth classes outside [0, K)."""
import ctypes as C

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import RsError, Trainer
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights, trainable_layers
from tests.test_gpu_trainer import _d2_grad, _engine_step, _oracle_losses_on_engine_samples
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu

NAMES = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
P_BOX, P_MASK = "roi_heads.box_predictor", "roi_heads.mask_head.predictor16"

# three boxes in image 0, four in image 1 (network-input pixels, 320 x 320)
GT_BOXES = [np.array([[20.0, 30.0, 120.0, 160.0], [150.0, 40.0, 300.0, 130.0], [60.0, 200.0, 110.0, 260.0]], np.float32),
            np.array([[100.0, 100.0, 260.0, 280.0], [10.0, 10.0, 60.0, 50.0], [200.0, 20.0, 300.0, 90.0], [20.0, 200.0, 90.0, 300.0]], np.float32)]
# classes 0 and K-1 always, at K = 8 also one of 3..6; at K = 4 class 2 and at K = 8 classes 1, 3, 5, 6 have NO box: their rows of the
# two predictors must come out exactly zero
GT_CLASSES = {1: ([0, 0, 0], [0, 0, 0, 0]), 3: ([0, 2, 1], [2, 0, 1, 2]), 4: ([0, 3, 1], [3, 0, 1, 3]), 8: ([0, 7, 4], [7, 2, 0, 4])}


def _rows(K):
    return (5 * K + 1 + 15) // 16 * 16


def _problem(K):
    def blob(b, k):            # a k-gon inscribed in the box (partial masks inside jittered proposals)
        cx, cy, rx, ry = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2, (b[2] - b[0]) / 2, (b[3] - b[1]) / 2
        th = np.linspace(0, 2 * np.pi, k, endpoint=False)
        return [np.stack([cx + rx * np.cos(th), cy + ry * np.sin(th)], 1).reshape(-1)]
    polys = [[blob(b, 7 + i) for i, b in enumerate(bs)] for bs in GT_BOXES]
    return GT_BOXES, [np.array(c) for c in GT_CLASSES[K]], polys


def _spec(K, precision):
    return EngineSpec(num_classes=K, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision=precision)


def _torch_weights(Wn, grad):
    from oracle import train_oracle as T
    W = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32).clone() for k, v in Wn.items()}
    if grad:
        for k in T.trainable_keys(W):
            W[k].requires_grad_(True)
    return W


@pytest.fixture(scope="module", params=[(1, "fp32"), (3, "fp32"), (4, "fp32"), (8, "fp32"), (8, "fp16")], ids=lambda p: f"K{p[0]}-{p[1]}")
def step(request, gpu_required):
    """One training step of a K-class trainer and autograd of the oracle on its samples; everything the tests read is copied to the host."""
    K, precision = request.param
    spec = _spec(K, precision)
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem(K)
    scale = 1.0 if precision == "fp32" else 128.0
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=scale)
    try:
        tr.set_sampling(256, 0.5, 128, 0.25)
        targets, where = _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=5)
        W = _torch_weights(Wn, grad=True)
        losses, ref = _oracle_losses_on_engine_samples(tr, spec, W, gt_boxes, polys, targets, where)
        sum(ref[n] for n in NAMES).backward()
        layers = trainable_layers(spec)
        out = dict(K=K, precision=precision, spec=spec, scale=scale, W=W, tr=tr, layers=layers,
                   losses=np.array(losses[:5], np.float64), ref=[float(ref[n].detach()) for n in NAMES],
                   g={l: tr.tensor(f"g:{l}.w") / np.float32(scale) for l in layers},
                   gb={l: tr.tensor(f"g:{l}.b") / np.float32(scale) for l in (P_BOX, P_MASK)},
                   d_box_pred=tr.tensor("d:box_pred").astype(np.float32), roi_classes=tr.tensor("roi_classes"),
                   count=tr.tensor("roi_sampled_count"), mask_classes=tr.tensor("mask_classes")[:int(tr.tensor("mask_total")[0])])
        yield out
    finally:
        tr.close()


def test_sampled_classes_cover_the_range(step):
    """Not vacuous: class K-1 and at least min(K, 3) distinct classes are among the mask-head entries (= the sampled foreground RoIs)."""
    K, mc, rc, cnt = step["K"], step["mask_classes"], step["roi_classes"], step["count"]
    fg = np.concatenate([rc[i, :int(cnt[i, 0])] for i in range(2)])
    print(f"K={K} {step['precision']}: sampled fg/bg per image {cnt.tolist()}, mask-entry classes {np.bincount(mc, minlength=K).tolist()}")
    assert np.array_equal(np.sort(fg), np.sort(mc))
    assert mc.min() >= 0 and mc.max() == K - 1 and len(np.unique(mc)) >= min(K, 3)
    for i in range(2):
        k = int(cnt[i].sum())
        assert (rc[i, int(cnt[i, 0]):k] == K).all() and (rc[i, k:] == -1).all()          # background label K, empty slots -1


def test_five_losses_and_every_weight_gradient_match_autograd(step):
    """The bounds tests/test_gpu_trainer.py holds at K = 2.  fp32: losses 1e-4 |ref| + 1e-7, every trainable layer's weight gradient
    <= 1e-3 relative L2 (measured worst at K = 2: 4.6e-4, ReLU masks of near-zero activations flipping).  fp16: losses 1.5e-2, the head
    tensors (roi_heads.*, proposal_generator.*, fpn_output2/3) <= 4e-2 and res4.2.conv2 <= 8e-2.  The predictors' bias gradients and --
    in fp32 -- every class' own rows of the two predictors are held to the same bound: a rare class' rows are a small part of the
    tensor's norm."""
    K, f32, W, spec = step["K"], step["precision"] == "fp32", step["W"], step["spec"]
    for i, n in enumerate(NAMES):
        got, r = float(step["losses"][i]), step["ref"][i]
        print(f"K={K} {step['precision']} {n}: engine {got:.8g} oracle {r:.8g} rel {abs(got - r) / abs(r):.2e}")
        assert abs(got - r) <= ((1e-4 * abs(r) + 1e-7) if f32 else (1.5e-2 * abs(r) + 1e-6)), (n, got, r)

    def rel(got, want):
        assert got.shape == want.shape, (got.shape, want.shape)
        return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
    want = {l: _d2_grad(W, l, spec) for l in step["layers"]}
    assert want[P_BOX].shape == (_rows(K), 1024) and want[P_MASK].shape == (16, 256)
    worst = {l: rel(step["g"][l], want[l]) for l in step["layers"]}
    p = "roi_heads.box_predictor."
    wb = np.zeros(_rows(K), np.float32)
    wb[:5 * K + 1] = torch.cat([W[p + "cls_score.bias"].grad, W[p + "bbox_pred.bias"].grad]).numpy()
    wm = np.zeros(16, np.float32)
    wm[:K] = W["roi_heads.mask_head.predictor.bias"].grad.numpy()
    worst[P_BOX + ".b"], worst[P_MASK + ".b"] = rel(step["gb"][P_BOX], wb), rel(step["gb"][P_MASK], wm)
    blocks = {}
    for c in np.unique(step["mask_classes"]):
        r4 = slice(K + 1 + 4 * c, K + 5 + 4 * c)
        blocks[f"bbox_pred[{c}]"] = rel(step["g"][P_BOX][r4], want[P_BOX][r4])
        blocks[f"mask_predictor[{c}]"] = rel(step["g"][P_MASK][c:c + 1], want[P_MASK][c:c + 1])
    for c in range(K + 1):
        blocks[f"cls_score[{c}]"] = rel(step["g"][P_BOX][c:c + 1], want[P_BOX][c:c + 1])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print(f"K={K} {step['precision']} worst weight-gradient rel L2:", [(k.split(".", 2)[-1], f"{v:.2e}") for k, v in top])
    print(f"K={K} {step['precision']} per-class rows:", {k: f"{v:.2e}" for k, v in blocks.items()})
    if f32:
        assert max(worst.values()) <= 1e-3, top
        assert max(blocks.values()) <= 1e-3, blocks
    else:
        heads = {k: v for k, v in worst.items() if k.startswith(("roi_heads.", "proposal_generator.")) or k in ("backbone.fpn_output2", "backbone.fpn_output3")}
        assert len(heads) >= 14 and max(heads.values()) <= 4e-2, sorted(heads.items(), key=lambda kv: -kv[1])[:6]
        assert worst["backbone.bottom_up.res4.2.conv2"] <= 8e-2


def test_padding_rows_and_absent_classes_are_exactly_zero(step):
    """Exact, in both precisions: rows >= 5K+1 of the box predictor's and rows >= K of the mask predictor's gradients (weights and
    biases) are 0; a class without a sampled foreground RoI has 0 in its mask-predictor row and its four bbox_pred rows, a class with
    one has non-zero weight rows there; the 64-wide gradient of the predictor output is 0 from column 5K+1 on."""
    K = step["K"]
    gw, gb, mw, mb = step["g"][P_BOX], step["gb"][P_BOX], step["g"][P_MASK], step["gb"][P_MASK]
    assert gw.shape == (_rows(K), 1024) and gb.shape == (_rows(K),) and mw.shape == (16, 256) and mb.shape == (16,)
    assert not gw[5 * K + 1:].any() and not gb[5 * K + 1:].any()
    assert not mw[K:].any() and not mb[K:].any()
    d = step["d_box_pred"]
    assert d.shape == (2, 1024, 64) and not d[:, :, 5 * K + 1:].any() and d[:, :, :5 * K + 1].any()
    present = set(int(c) for c in step["mask_classes"])
    assert present <= set(range(K))
    if K in (4, 8):
        assert len(present) < K                   # the zero-row branch below is exercised
    for c in range(K):
        r4 = slice(K + 1 + 4 * c, K + 5 + 4 * c)
        if c in present:
            assert mw[c].any() and mb[c] != 0 and gw[r4].any(axis=1).all(), c          # (a bbox_pred bias gradient is a sum of +-1 / n: it may cancel)
        else:
            assert not mw[c].any() and mb[c] == 0 and not gw[r4].any() and not gb[r4].any(), c
    assert gw[:K + 1].any(axis=1).all() and (gb[:K + 1] != 0).all()          # every class logit, background included


def test_ground_truth_classes_outside_the_range_are_refused(step):
    """rs_trainer_set_targets validates the classes of the counted boxes: class K (the background label) and class -1 are RS_ERR_ARG,
    surfaced as RsError naming the image, the box index, the class and the range; the padding slots beyond gt_count[i] are not looked
    at.  (Unchecked, class K counted in n_valid while box_loss_kernel dropped it, and any class < 16 trained a padding channel of the
    16-row mask predictor; detectron2's cross_entropy rejects such a target.)"""
    K, tr = step["K"], step["tr"]
    boxes = [GT_BOXES[0][:2], GT_BOXES[1][:3]]
    for bad, img, idx in ((K, 1, 2), (-1, 0, 1)):
        cls = [np.zeros(2, np.int64), np.zeros(3, np.int64)]
        cls[img][idx] = bad
        with pytest.raises(RsError) as e:
            tr.set_targets(boxes, cls)
        msg = str(e.value)
        assert f"image {img}" in msg and f"box {idx}" in msg and f"class {bad}" in msg and f"[0, {K})" in msg, msg
    tr.set_targets(boxes, [np.full(2, K - 1), np.full(3, K - 1)])
    # through the C ABI: garbage in the slots past the counts is ignored
    cap = 4
    bx = np.zeros((2, cap, 4), np.float32)
    bx[0, :2], bx[1, :3] = boxes[0], boxes[1]
    cl = np.array([[0, K - 1, 99, -7], [K - 1, 0, 0, K]], np.int32)
    cnt = np.array([2, 3], np.int32)
    vp = C.c_void_p
    assert tr.lib.rs_trainer_set_targets(tr._h, bx.ctypes.data_as(vp), cl.ctypes.data_as(vp), cnt.ctypes.data_as(vp), 2, cap) == 0
    cnt[1] = 4
    assert tr.lib.rs_trainer_set_targets(tr._h, bx.ctypes.data_as(vp), cl.ctypes.data_as(vp), cnt.ctypes.data_as(vp), 2, cap) != 0
    assert f"image 1, box 3: ground-truth class {K}" in tr.lib.rs_last_error().decode()


def test_two_sgd_steps_keep_the_48_row_predictor_consistent(gpu_required):
    """K = 8, fp32: step, apply_sgd with the YAML's iteration-0 hyper-parameters, second step on the same tiles.  The 48-row master of
    the box predictor moves by the closed form, its rows >= 41 (and the mask predictor's rows >= 8) stay exactly 0, and the second
    step's five losses equal the oracle's on export_weights() at the fp32 bound -- the refold of a 48-row master and of mask-predictor
    rows 0..7 into every forward operand.  Iteration 0 is a warm-up step (lr 1e-5), too small for a STALE operand to show in a loss, so
    a third step follows an update at the YAML's BASE_LR."""
    from oracle import train_oracle as T
    K = 8
    spec = _spec(K, "fp32")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem(K)
    ts = T.TrainSpec()
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=1.0)
    try:
        tr.set_sampling(256, 0.5, 128, 0.25)
        _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=5)
        m0, g0 = tr.tensor(f"m:{P_BOX}.w").copy(), tr.tensor(f"g:{P_BOX}.w").copy()
        assert m0.shape == (48, 1024) and not m0[41:].any() and m0[:41].any(axis=1).all()
        for it, lr in enumerate((T.lr_at(ts, 0), ts.base_lr)):
            tr.apply_sgd(lr, ts.momentum, ts.weight_decay)
            tr.sync()
            m1 = tr.tensor(f"m:{P_BOX}.w")
            if it == 0:
                want = m0 - np.float32(lr) * (g0 + np.float32(ts.weight_decay) * m0)
                assert np.allclose(m1, want, rtol=1e-5, atol=1e-9) and float(np.abs(m1[:41] - m0[:41]).max()) > 0
            assert not m1[41:].any() and not tr.tensor(f"m:{P_BOX}.b")[41:].any()
            assert not tr.tensor(f"m:{P_MASK}.w")[K:].any() and not tr.tensor(f"m:{P_MASK}.b")[K:].any()
            targets, where = _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=6 + it)
            assert K - 1 in tr.tensor("mask_classes")[:int(tr.tensor("mask_total")[0])]
            W = _torch_weights(tr.export_weights(Wn), grad=False)
            with torch.no_grad():
                losses, ref = _oracle_losses_on_engine_samples(tr, spec, W, gt_boxes, polys, targets, where)
            for i, n in enumerate(NAMES):
                r = float(ref[n])
                print(f"after update {it} (lr {lr:g}) {n}: engine {float(losses[i]):.8g} oracle {r:.8g} rel {abs(float(losses[i]) - r) / abs(r):.2e}")
                assert abs(float(losses[i]) - r) <= 1e-4 * abs(r) + 1e-7, (it, n, float(losses[i]), r)
    finally:
        tr.close()
