"""MODEL.BACKBONE.FREEZE_AT 0 and 1 on the GPU (csrc/stem_bwd.hip, csrc/trainer.hip): the two stem-backward operators against their
numpy restatements (tests/freeze_at_ref.py), the assembled training step against autograd of the oracle at the existing bars, the
invariants between the three values, the unchanged default, the split modes, the fp16 trainer and the command line."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import RsError, Trainer, _check, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import conv_layers, synthetic_weights, trainable_layers
from tests import freeze_at_ref as R
from tests.test_freeze_at_cpu import pool_inputs
from tests.test_gpu_trainer import _d2_grad, _engine_step, _tiny_training_workdir, _two_image_problem
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu
STEM = "backbone.bottom_up.stem.conv1"
NAMES = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")


def _halo(a: np.ndarray, pad: int, fill=0.0) -> np.ndarray:
    n, h, w, c = a.shape
    out = np.full((n, h + 2 * pad, w + 2 * pad, c), fill, a.dtype)
    out[:, pad:pad + h, pad:pad + w] = a
    return out


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ pool backward operator
def run_pool_bwd(x: np.ndarray, dq: np.ndarray, f32: bool) -> np.ndarray:
    """d_stem_conv [n][h+2][w+2][c] with its halo, the output buffer pre-filled with NaN."""
    lib = load_library()
    dt = torch.float32 if f32 else torch.float16
    dev = torch.device("cuda:0")
    n, h, w, c = x.shape
    xd = torch.from_numpy(_halo(x, 1)).to(dt).to(dev)
    qd = torch.from_numpy(_halo(dq, 1)).to(dt).to(dev)
    od = torch.full(xd.shape, float("nan"), dtype=dt, device=dev)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_maxpool3x3s2_bwd(_ptr(xd), _ptr(qd), _ptr(od), n, h, w, c, 1, 1, 1 if f32 else 0, None), "rs_op_maxpool3x3s2_bwd")
    torch.cuda.synchronize()
    return od.float().cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("kind", ["ties", "continuous"])
@pytest.mark.parametrize("hw", [(8, 12), (6, 6), (7, 9)])
def test_pool_backward_operator(gpu_required, f32, kind, hw):
    """Interior equal to the restatement bit for bit (fp16 storage: after the kernel's one final rounding), the halo untouched, two
    calls the same bits.  (7, 9): odd sizes, where the last row / column of pixels has no partner in its 2 x 2 block."""
    h, w = hw
    x, dq = pool_inputs(kind, 2, h, w, 64, seed=h * 100 + w + (7 if f32 else 0))
    want = R.maxpool_relu_bwd(x, dq)
    if not f32:
        want = want.astype(np.float16).astype(np.float32)
    got = run_pool_bwd(x, dq, f32)
    inner = got[:, 1:-1, 1:-1]
    assert np.array_equal(inner, want), float(np.abs(inner - want).max())
    mask = np.ones(got.shape, bool)
    mask[:, 1:-1, 1:-1] = False
    assert np.isnan(got[mask]).all() and not np.isnan(inner).any()
    assert np.array_equal(run_pool_bwd(x, dq, f32)[:, 1:-1, 1:-1], inner)
    assert float((inner != 0).mean()) > 0.05


def test_pool_backward_operator_refuses_bad_arguments(gpu_required):
    lib = load_library()
    buf = torch.zeros(4096, device="cuda:0")
    assert lib.rs_op_maxpool3x3s2_bwd(None, _ptr(buf), _ptr(buf), 1, 4, 4, 8, 1, 1, 0, None) < 0
    assert lib.rs_op_maxpool3x3s2_bwd(_ptr(buf), _ptr(buf), _ptr(buf), 1, 4, 4, 12, 1, 1, 0, None) < 0       # 12 channels: no 16-byte pieces of fp16
    assert lib.rs_op_maxpool3x3s2_bwd(_ptr(buf), _ptr(buf), _ptr(buf), 1, 4, 4, 6, 1, 1, 1, None) < 0


# ------------------------------------------------------------------------------------------------ stem weight-gradient operator
def run_stem_wgrad(dy: np.ndarray, x0: np.ndarray, f32: bool, scale=None, splits=0, x_halo=3, dy_halo=1) -> np.ndarray:
    """grad [64][256] from dy [n][hc][wc][64] and x0 [n][2hc][2wc][cin]; x0 is stored with 4 channels, the missing ones filled with a
    non-zero value so that a kernel which did not mask them would show."""
    lib = load_library()
    dt = torch.float32 if f32 else torch.float16
    dev = torch.device("cuda:0")
    n, hc, wc, _ = dy.shape
    cin = x0.shape[3]
    x4 = np.full(x0.shape[:3] + (4,), 3.0, np.float32)
    x4[..., :cin] = x0
    xd = torch.from_numpy(_halo(x4, x_halo)).to(dt).to(dev)
    yd = torch.from_numpy(_halo(dy, dy_halo, fill=7.0)).to(dt).to(dev)          # the halo of dy is never read
    gd = torch.full((64, 256), float("nan"), dtype=torch.float32, device=dev)
    sd = torch.from_numpy(scale).to(dev) if scale is not None else None
    fn = lib.rs_op_stem_wgrad_f32 if f32 else lib.rs_op_stem_wgrad
    torch.cuda.synchronize()
    _check(lib, fn(_ptr(yd), _ptr(xd), _ptr(gd), _ptr(sd) if sd is not None else None, n, hc, wc, cin, dy_halo, x_halo, splits, None), "rs_op_stem_wgrad")
    torch.cuda.synchronize()
    return gd.cpu().numpy()


@pytest.mark.parametrize("f32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("cin,n,hw,scaled,splits", [
    (3, 1, (8, 8), False, 1),        # one image, one split: every pixel through one workgroup
    (3, 3, (12, 6), True, 4),        # several splits, a row of 6 pixels: steps of 4 pixels straddle rows and images
    (4, 3, (8, 8), True, 0),         # four bands, the library's own split count
    (4, 1, (12, 6), False, 5),       # 18 steps over 5 splits: the last split is short
    (3, 1, (8, 8), True, 16),        # one step per split
])
def test_stem_wgrad_operator(gpu_required, f32, cin, n, hw, scaled, splits):
    """Per element against float64 in the form of test_gpu_train_ops.py::test_conv_wgrad_f32_matches_autograd (1e-5 of the largest
    entry: the products are exact in fp32 for both operand types, only the accumulation order differs); padding columns exactly zero;
    two calls the same bits."""
    hc, wc = hw
    rng = np.random.default_rng(cin * 1000 + n * 100 + hc + splits)
    r16 = (lambda a: a.astype(np.float16).astype(np.float32)) if not f32 else (lambda a: a)
    dy = r16((rng.standard_normal((n, hc, wc, 64)) * 0.1).astype(np.float32))
    x0 = r16(rng.standard_normal((n, 2 * hc, 2 * wc, cin)).astype(np.float32))
    scale = (rng.random(64) + 0.5).astype(np.float32) * np.where(np.arange(64) % 5 == 0, -1, 1).astype(np.float32) if scaled else None
    ref, _ = R.stem_wgrad(dy, x0, scale)
    got = run_stem_wgrad(dy, x0, f32, scale=scale, splits=splits)
    pad = R.stem_padding_mask() | (np.arange(256) % 4 >= cin)
    assert np.all(got[:, pad] == 0) and not np.signbit(got[:, pad]).any(), "padding columns must be +0"
    err = float(np.abs(got - ref).max())
    print(f"stem wgrad cin {cin} n {n} {hc}x{wc} splits {splits}: max err {err:.3e}, ref max {float(np.abs(ref).max()):.3e}")
    assert err <= 1e-5 * max(1.0, float(np.abs(ref).max())), f"max err {err}, ref max {float(np.abs(ref).max())}"
    assert float(np.abs(ref[:, ~pad]).min()) > 0 and np.all(got[:, ~pad] != 0)
    assert np.array_equal(run_stem_wgrad(dy, x0, f32, scale=scale, splits=splits), got)


def test_stem_wgrad_operator_wide_halos(gpu_required):
    """Halos other than the engine's (input 4, gradient 0) address the same pixels."""
    rng = np.random.default_rng(5)
    dy = (rng.standard_normal((2, 8, 8, 64)) * 0.1).astype(np.float32)
    x0 = rng.standard_normal((2, 16, 16, 3)).astype(np.float32)
    a = run_stem_wgrad(dy, x0, True, splits=2)
    b = run_stem_wgrad(dy, x0, True, splits=2, x_halo=4, dy_halo=0)
    assert np.array_equal(a, b)


def test_stem_wgrad_operator_refuses_bad_arguments(gpu_required):
    lib = load_library()
    buf = torch.zeros(1 << 16, device="cuda:0")
    ok = (1, 8, 8, 3, 1, 3, 0)
    assert lib.rs_op_stem_wgrad_f32(_ptr(buf), _ptr(buf), None, None, *ok, None) < 0
    for bad in ((1, 8, 8, 5, 1, 3, 0), (1, 8, 8, 3, 1, 2, 0), (1, 8, 8, 3, 1, 3, 513), (0, 8, 8, 3, 1, 3, 0)):
        assert lib.rs_op_stem_wgrad_f32(_ptr(buf), _ptr(buf), _ptr(buf), None, *bad, None) < 0, bad
        assert "rs_op_stem_wgrad" in lib.rs_last_error().decode()


# ------------------------------------------------------------------------------------------------ assembled step
def _spec(precision: str, bands: int) -> EngineSpec:
    kw = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision=precision)
    if bands == 4:
        kw.update(pixel_mean=(103.53, 116.28, 123.675, 110.0), pixel_std=(1.0, 1.0, 1.0, 1.0))
    return EngineSpec(**kw)


def _stem_layout(g: np.ndarray) -> np.ndarray:
    """(64, C, 7, 7) -> the stem's [64][256] GEMM layout."""
    out = np.zeros((g.shape[0], 7, 8, 4), np.float32)
    out[:, :, :7, :g.shape[1]] = g.transpose(0, 2, 3, 1)
    return np.concatenate([out.reshape(g.shape[0], 224), np.zeros((g.shape[0], 32), np.float32)], 1)


def _oracle_losses(tr, spec, W, gt_boxes, polys, targets, where, bands):
    """tests/test_gpu_trainer.py::_oracle_losses_on_engine_samples for a network input of ``bands`` channels: the five losses of the
    oracle on the engine's own network input, sampled anchors and sampled RoIs."""
    from oracle import maskrcnn_oracle as O
    from oracle import train_oracle as T
    cnt = tr.tensor("roi_sampled_count")
    assert int(tr.tensor("mask_total")[0]) == len(where) == int(cnt[:, 0].sum()) and len(where) >= 3
    boxes, cls, gtb, gti = tr.tensor("roi_boxes"), tr.tensor("roi_classes"), tr.tensor("roi_gt_boxes"), tr.tensor("roi_gt_index")
    K = spec.num_classes
    x = torch.from_numpy(tr.tensor("net_input", engine=True)[..., :bands].astype(np.float32)).permute(0, 3, 1, 2)
    feats = O.resnet_forward(spec, W, x)
    feats.update(O.fpn_forward(spec, W, feats))
    logits, deltas = O.rpn_head(W, [feats[n] for n in spec.rpn_in_features])
    lg = torch.cat([t.permute(0, 2, 3, 1).reshape(2, -1) for t in logits], 1)
    dl = torch.cat([t.view(2, -1, 4, t.shape[2], t.shape[3]).permute(0, 3, 4, 1, 2).reshape(2, -1, 4) for t in deltas], 1)
    anchors = torch.cat([O.grid_anchors(spec, l, hw, hw) for l, hw in enumerate((80, 40, 20, 10, 5))])
    labels = torch.from_numpy(tr.tensor("rpn_labels").astype(np.int64))
    matched = torch.from_numpy(tr.tensor("rpn_matched").astype(np.int64))
    ts = T.TrainSpec()
    ref = T.rpn_losses(anchors, lg, dl, [labels[0].to(torch.int8), labels[1].to(torch.int8)],
                       [torch.from_numpy(gt_boxes[i])[matched[i]] for i in range(2)], ts)
    rb, rc, rg, ri = [], [], [], []
    for i in range(2):
        k = int(cnt[i].sum())
        c = cls[i, :k]
        rb.append(torch.from_numpy(boxes[i, :k])); rc.append(torch.from_numpy(c.astype(np.int64)))
        rg.append(torch.from_numpy(np.where((c < K)[:, None], gtb[i, :k], boxes[i, :k]))); ri.append(torch.full((k,), i, dtype=torch.int64))
    rb, rc, rg, ri = torch.cat(rb), torch.cat(rc), torch.cat(rg), torch.cat(ri)
    roi_feats = [feats[n] for n in spec.roi_in_features]
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    _, scores, reg = O.box_head(W, T.roi_pooler_diff(roi_feats, scales, rb, ri, 7))
    ref.update(T.fast_rcnn_losses(scores, reg, rb, rc, rg, K, spec.box_reg_weights, ts))
    mb = torch.from_numpy(np.stack([boxes[i, j] for i, j in where]))
    mi = torch.tensor([i for i, _ in where])
    mc = torch.tensor([int(cls[i, j]) for i, j in where])
    mlog, _ = O.mask_head(spec, W, T.roi_pooler_diff(roi_feats, scales, mb, mi, 14), mc)
    gm = torch.from_numpy(np.stack([T.rasterize_polygons_within_box(polys[i][int(gti[i, j])], boxes[i, j], 28) for i, j in where]))
    assert np.array_equal(gm.numpy(), targets)
    ref["loss_mask"] = T.mask_rcnn_loss(mlog, mc, gm)
    return ref


@functools.lru_cache(maxsize=None)
def step(precision: str, freeze_at, bands: int = 3, split: bool = False, oracle: bool = False, sgd: bool = False, run: int = 0):
    """One training step of a fresh trainer on the two-image problem of tests/test_gpu_trainer.py (``freeze_at`` None: the argument is
    not passed), computed once per argument set and shared by the tests below, which only read it.  ``oracle``: autograd of the oracle
    on the engine's samples with EVERY backbone tensor trainable, and with ``sgd`` its torch.optim.SGD step; ``sgd``: apply_sgd after
    the gradients were read, then export the weights.  ``run``: a second value gives a second, independent run of the same step."""
    from oracle import train_oracle as T
    spec = _spec(precision, bands)
    Wn = synthetic_weights(_spec(precision, 3), seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    if bands == 4:
        # The three-band problem with a fourth band added the way a detector is fine-tuned from a three-band checkpoint: the stem gains
        # an input channel that starts at zero, the tiles gain a band.  The forward is then the three-band one value for value, so the
        # step draws the same samples, and what is new is the gradient of the fourth channel.  (Model channel c reads source channel
        # C - 1 - c for the RGB input format: the new band is the FIRST source channel.)
        w = np.asarray(Wn[STEM + ".weight"])
        Wn = dict(Wn)
        Wn[STEM + ".weight"] = np.concatenate([w, np.zeros((64, 1, 7, 7), w.dtype)], 1)
        band = synthetic_tiles(2, 256, 256, 4, seed=778)[..., :1]
        tiles = np.concatenate([band, tiles] if spec.input_format == "RGB" else [tiles, band], -1)
    gt_boxes, gt_classes, polys = _two_image_problem()
    scale = 1.0 if precision == "fp32" else 128.0
    kw = {} if freeze_at is None else {"freeze_at": freeze_at}
    if split:
        kw.update(wgrad="split", dgrad="split", fwd="split")
    fa = 2 if freeze_at is None else freeze_at
    out = types.SimpleNamespace(spec=spec, Wn=Wn, scale=scale, freeze_at=fa)
    ts = T.TrainSpec()
    tr = Trainer(spec, Wn, (256, 256, bands), batch=2, loss_scale=scale, **kw)
    try:
        assert tr.freeze_at == fa and tr.lib.rs_trainer_freeze_at(tr._h) == fa
        tr.set_sampling(256, 0.5, 64, 0.25)
        targets, where = _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=5)
        out.losses = tr.tensor("losses").copy()
        out.layers = trainable_layers(spec, fa)
        out.grads = {l: tr.tensor(f"g:{l}.w").copy() for l in out.layers}
        out.samples = {k: tr.tensor(k).copy() for k in ("rpn_labels", "roi_boxes", "roi_classes", "roi_sampled_count")}
        out.buckets = tr.buckets()
        out.param_count = tr.param_count
        out.tensor_names = tr.tensor_names()
        tr.set_profiling(False)                      # builds the stage list; nothing is timed
        out.stage_names = [s["name"] for s in tr.stage_times()]
        if oracle:
            W = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32).clone() for k, v in Wn.items()}
            keys = T.trainable_keys(W, 0)
            for k in keys:
                W[k].requires_grad_(True)
            ref = _oracle_losses(tr, spec, W, gt_boxes, polys, targets, where, bands)
            opt = torch.optim.SGD([W[k] for k in keys], lr=T.lr_at(ts, 0), momentum=ts.momentum, weight_decay=ts.weight_decay)
            sum(ref[n] for n in NAMES).backward()
            out.ref_losses = {n: float(ref[n].detach()) for n in NAMES}
            out.ref_grads = {l: (_stem_layout(W[l + ".weight"].grad.numpy()) if l == STEM else _d2_grad(W, l, spec)).copy()
                             for l in trainable_layers(spec, 0)}
            if sgd:
                opt.step()
                out.ref_weights = {k: W[k].detach().numpy().copy() for k in keys}
        if sgd:
            tr.apply_sgd(T.lr_at(ts, 0), ts.momentum, ts.weight_decay)
            tr.sync()
            out.exported = tr.export_weights(Wn)
    finally:
        tr.close()
    return out


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def _check_fp32_bars(run, ref, what):
    """The bars of test_reference_precision_training_step_matches_autograd: losses to 1e-4, every weight gradient to 1e-3 relative L2."""
    for i, n in enumerate(NAMES):
        r = ref.ref_losses[n]
        assert abs(float(run.losses[i]) - r) <= 1e-4 * abs(r) + 1e-7, (what, n, float(run.losses[i]), r)
    worst = {}
    for layer in run.layers:
        assert run.grads[layer].shape == ref.ref_grads[layer].shape, (layer, run.grads[layer].shape, ref.ref_grads[layer].shape)
        worst[layer] = _rel(run.grads[layer], ref.ref_grads[layer])
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    new = [(k.split(".", 2)[-1], f"{v:.2e}") for k, v in top if ".res2." in k or ".stem." in k]
    old = [(k.split(".", 2)[-1], f"{v:.2e}") for k, v in top if not (".res2." in k or ".stem." in k)][:1]
    print(f"{what}: weight-gradient rel L2 of the new tensors {new}; worst of the tensors trained at FREEZE_AT 2 {old}")
    assert top[0][1] <= 1e-3, top[:6]
    return worst


def test_fp32_step_at_0_matches_autograd(gpu_required):
    """Losses and every weight gradient -- stem.conv1 and all of res2 included -- at the existing bars."""
    a = step("fp32", 0, oracle=True, sgd=True)
    assert STEM in a.layers and sum(".res2." in l for l in a.layers) == 10
    worst = _check_fp32_bars(a, a, "fp32 trainer, FREEZE_AT 0")
    assert worst[STEM] > 0 and float(np.abs(a.grads[STEM]).max()) > 0
    pad = R.stem_padding_mask() | (np.arange(256) % 4 >= 3)
    assert np.all(a.grads[STEM][:, pad] == 0)


def test_fp32_step_at_1_matches_autograd(gpu_required):
    """The forward of the fp32 trainer does not depend on freeze_at, so the step at 1 draws the samples of the step at 0 and is
    compared with the same autograd run."""
    a, b = step("fp32", 0, oracle=True, sgd=True), step("fp32", 1, sgd=True)
    for k in a.samples:
        assert np.array_equal(a.samples[k], b.samples[k]), k
    assert STEM not in b.layers and sum(".res2." in l for l in b.layers) == 10
    _check_fp32_bars(b, a, "fp32 trainer, FREEZE_AT 1")


def test_fp32_step_with_four_bands(gpu_required):
    """A 4-band detector at FREEZE_AT 0: the fourth input channel's stem gradient is there and inside the bar on its own.  The problem
    is the three-band one with a zero-initialised fourth stem channel (see ``step``), so everything but that channel's gradient must
    also equal the three-band run bit for bit.

    Measured before this form was chosen, with synthetic_weights of the 4-band spec and 4-band synthetic tiles (another forward,
    other samples): stem.conv1 1.15e-3 and the worst res2 tensor 1.02e-3 beside 1.78e-3 for res3.1.conv2 and 1.71e-3 for res3.1.conv1,
    tensors the trainer already trains at FREEZE_AT 2 through unchanged code -- that draw exceeds the 1e-3 bar above the stem too,
    so it says nothing about the new stages and is not used as the case."""
    a, c = step("fp32", 0, oracle=True, sgd=True), step("fp32", 0, bands=4, oracle=True)
    for k in a.samples:
        assert np.array_equal(a.samples[k], c.samples[k]), k
    assert np.array_equal(a.losses, c.losses)
    for l in a.layers:
        if l != STEM:
            assert np.array_equal(a.grads[l], c.grads[l]), l
    assert np.array_equal(a.grads[STEM][:, np.arange(256) % 4 < 3], c.grads[STEM][:, np.arange(256) % 4 < 3])
    _check_fp32_bars(c, c, "fp32 trainer, 4 bands, FREEZE_AT 0")
    ch3 = np.arange(256) % 4 == 3
    got, want = c.grads[STEM][:, ch3], c.ref_grads[STEM][:, ch3]
    assert float(np.abs(want).max()) > 0 and float(np.abs(got).max()) > 0
    r = _rel(got, want)
    print(f"4-band stem gradient, fourth channel alone: rel L2 {r:.2e}")
    assert r <= 1e-3
    assert np.all(c.grads[STEM][:, R.stem_padding_mask()] == 0)


def test_values_0_and_1_agree_bit_for_bit_above_the_stem(gpu_required):
    a, b = step("fp32", 0, oracle=True, sgd=True), step("fp32", 1, sgd=True)
    assert np.array_equal(a.losses, b.losses)
    assert [l for l in a.layers if l != STEM] == b.layers
    for l in b.layers:
        assert np.array_equal(a.grads[l], b.grads[l]), l


def test_value_2_agrees_with_1_from_res3_up(gpu_required):
    b, d = step("fp32", 1, sgd=True), step("fp32", 2)
    assert np.array_equal(b.losses, d.losses)
    assert [l for l in b.layers if ".res2." not in l] == d.layers
    for l in d.layers:
        assert np.array_equal(b.grads[l], d.grads[l]), l


def test_sgd_moves_what_is_trained_and_matches_the_oracle_step(gpu_required):
    """At 1 the stem's exported weight is bit-unchanged and res2's has moved; at 0 the stem's has moved.  The stem update at 0 and the
    res2 updates at 1 against torch.optim.SGD on the oracle's gradients, at the bars of test_twenty_sgd_steps_side_by_side_with_the_oracle
    (weights 1e-4, updates 2e-2 relative L2)."""
    a, b = step("fp32", 0, oracle=True, sgd=True), step("fp32", 1, sgd=True)
    sk = STEM + ".weight"
    w0 = np.asarray(a.Wn[sk], np.float32)
    assert a.exported[sk].shape == (64, 3, 7, 7) and b.exported[sk].shape == (64, 3, 7, 7)
    assert np.array_equal(b.exported[sk], w0)
    assert not np.array_equal(a.exported[sk], w0)
    res2 = [n + ".weight" for n, _, _, _, _ in conv_layers(a.spec) if ".res2." in n]
    for run, keys in ((a, [sk]), (b, res2)):
        for k in keys:
            w0, wo, we = np.asarray(run.Wn[k], np.float32), a.ref_weights[k], np.asarray(run.exported[k], np.float32)
            assert not np.array_equal(we, w0), k
            d = float(np.linalg.norm(wo - w0))
            rw, ru = _rel(we, wo), float(np.linalg.norm((we - w0) - (wo - w0)) / d)
            assert d > 0 and rw <= 1e-4 and ru <= 2e-2, (k, rw, ru)
    for k, v in a.exported.items():                     # nothing else changed shape or went missing
        assert v.shape == np.asarray(a.Wn[k]).shape, k


def test_two_runs_at_0_give_the_same_bits(gpu_required):
    a = step("fp32", 0, oracle=True, sgd=True)
    a2 = step("fp32", 0, sgd=True, run=1)
    assert a2 is not a
    assert np.array_equal(a.losses, a2.losses)
    for l in a.layers:
        assert np.array_equal(a.grads[l], a2.grads[l]), l
    for k in a.exported:
        assert np.array_equal(a.exported[k], a2.exported[k]), k


def test_buckets_at_each_value(gpu_required):
    for run, last in ((step("fp32", 2), "res3"), (step("fp32", 1, sgd=True), "res2"), (step("fp32", 0, oracle=True, sgd=True), "stem")):
        names = [b[0] for b in run.buckets]
        assert names == ["heads", "fpn", "res5", "res4", "res3", "res2", "stem"][:len(names)] and names[-1] == last, names
        spans = sorted((o, o + c) for _, o, c in run.buckets)
        assert spans[0][0] == 0 and spans[-1][1] == run.param_count and all(x[1] == y[0] for x, y in zip(spans, spans[1:])), spans
    assert step("fp32", 0, oracle=True, sgd=True).param_count == step("fp32", 1, sgd=True).param_count + 64 * 256
    assert step("fp32", 0, oracle=True, sgd=True).stage_names[-2:] == ["bwd.stem.maxpool", "bwd.stem.conv1.w"]
    assert "bwd.res2.0.shortcut.x" in step("fp32", 0, oracle=True, sgd=True).stage_names
    assert "bwd.res2.0.shortcut.w" in step("fp32", 1, sgd=True).stage_names and "bwd.res2.0.shortcut.x" not in step("fp32", 1, sgd=True).stage_names


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_explicit_2_is_the_default_trainer(gpu_required, precision):
    """Stage names, tensor names, bucket table and one step's loss and gradient bits."""
    d, e = step(precision, None), step(precision, 2)
    assert d.stage_names == e.stage_names and d.tensor_names == e.tensor_names and d.buckets == e.buckets and d.param_count == e.param_count
    assert [b[0] for b in d.buckets] == ["heads", "fpn", "res5", "res4", "res3"]
    assert not any("res2" in n or "stem" in n for n in d.stage_names if n.startswith("bwd."))
    if precision == "fp16":                              # the frozen stem and res2 keep their fused launches
        assert "stem.conv1+maxpool" in d.stage_names and any(n.startswith("res2.") and "+" in n for n in d.stage_names)
    assert np.array_equal(d.losses, e.losses)
    for l in d.layers:
        assert np.array_equal(d.grads[l], e.grads[l]), l


def test_fp16_forward_is_unfused_where_it_is_differentiated(gpu_required):
    s1, s0 = step("fp16", 1).stage_names, step("fp16", 0, oracle=True).stage_names
    assert "stem.conv1+maxpool" in s1 and not any(n.startswith("res2.") and "+" in n for n in s1)
    assert "stem.conv1" in s0 and "stem.maxpool" in s0 and "stem.conv1+maxpool" not in s0
    for s in (s0, s1):
        assert all(f"res2.{b}.conv{c}" in s for b in range(3) for c in (1, 2, 3)) and "res2.0.shortcut" in s


def test_split_modes_at_0(gpu_required):
    """wgrad, dgrad and fwd all "split": the same bars (the stem's three stages stay fp32 in every mode)."""
    s = step("fp32", 0, split=True, oracle=True)
    _check_fp32_bars(s, s, "fp32 trainer, FREEZE_AT 0, all three split modes")


def test_fp16_step_at_0(gpu_required):
    """The fp16 trainer's bars (test_full_training_step_five_losses_match_autograd): losses 1.5e-2, backbone gradients 8e-2 relative
    L2 -- on stem.conv1 and every res2 tensor."""
    h = step("fp16", 0, oracle=True)
    for i, n in enumerate(NAMES):
        r = h.ref_losses[n]
        assert abs(float(h.losses[i]) - r) <= 1.5e-2 * abs(r) + 1e-6, (n, float(h.losses[i]), r)
    worst = {l: _rel(h.grads[l] / h.scale, h.ref_grads[l]) for l in h.layers if ".res2." in l or l == STEM}
    print("fp16 trainer, FREEZE_AT 0: weight-gradient rel L2 of the new tensors", {k.split(".", 2)[-1]: round(v, 4) for k, v in worst.items()})
    assert len(worst) == 11 and max(worst.values()) <= 8e-2, worst
    pad = R.stem_padding_mask() | (np.arange(256) % 4 >= 3)
    assert np.all(h.grads[STEM][:, pad] == 0)


def test_create2_refuses_other_values_and_mixed_copy_state(gpu_required):
    from proj_roadsurf_amd.engine import RsSpec, RsTrainOptions, make_rs_spec
    from proj_roadsurf_amd.weights import pack_weights
    lib = load_library()
    spec = EngineSpec(num_classes=2, min_size_test=128, max_size_test=213, precision="fp32")
    W = synthetic_weights(spec, seed=0)
    blob = pack_weights(spec, W, train=True, freeze_at=0)
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    rs = make_rs_spec(spec)
    vp, i32 = C.c_void_p, C.c_int
    lib.rs_trainer_create2.argtypes = [C.POINTER(RsSpec), vp, C.c_size_t, i32, i32, i32, i32, i32, C.c_float, C.POINTER(RsTrainOptions), C.POINTER(vp)]
    for bad in (3, 5, -1):
        h = C.c_void_p()
        opts = RsTrainOptions(C.sizeof(RsTrainOptions), bad)
        rc = lib.rs_trainer_create2(C.byref(rs), buf, len(blob), 0, 1, 128, 128, 3, 1.0, C.byref(opts), C.byref(h))
        assert rc == -4 and not h.value and "FREEZE_AT" in lib.rs_last_error().decode(), (bad, rc)
    h = C.c_void_p()
    opts = RsTrainOptions(4, 0)
    assert lib.rs_trainer_create2(C.byref(rs), buf, len(blob), 0, 1, 128, 128, 3, 1.0, C.byref(opts), C.byref(h)) == -1 and not h.value
    t0 = Trainer(spec, W, (128, 128, 3), batch=1, freeze_at=0)
    t1 = Trainer(spec, W, (128, 128, 3), batch=1, freeze_at=1)
    try:
        with pytest.raises(RsError, match="FREEZE_AT"):
            t1.copy_state_from(t0)
        # a blob packed for FREEZE_AT 2 lacks the master weights of res2: refused, not trained from something else
        blob2 = pack_weights(spec, W, train=True)
        buf2 = (C.c_char * len(blob2)).from_buffer_copy(blob2)
        opts = RsTrainOptions(C.sizeof(RsTrainOptions), 1)
        assert lib.rs_trainer_create2(C.byref(rs), buf2, len(blob2), 0, 1, 128, 128, 3, 1.0, C.byref(opts), C.byref(h)) < 0 and not h.value
    finally:
        t0.close()
        t1.close()


def test_train_model_cli_with_freeze_at_0(gpu_required, tmp_path):
    """FREEZE_AT: 0 in the YAML reaches the trainer: model_final.pth loads, its stem weight is (64, 3, 7, 7) and has moved."""
    import os

    import yaml

    from proj_roadsurf_amd import train_model
    from proj_roadsurf_amd.weights import load_checkpoint
    wd = _tiny_training_workdir(tmp_path)
    d2 = yaml.safe_load(open(tmp_path / "d2.yaml"))
    d2["MODEL"]["BACKBONE"] = {"FREEZE_AT": 0}
    d2["INPUT"]["MIN_SIZE_TRAIN"] = [160]
    d2["TEST"]["EVAL_PERIOD"] = 0
    yaml.safe_dump(d2, open(tmp_path / "d2.yaml", "w"))
    cwd = os.getcwd()
    try:
        assert train_model.main([str(tmp_path / "config.yaml"), "--synthetic-weights", "--max-iter", "2", "--log-period", "1", "--tagged-samples", "0"]) == 0
    finally:
        os.chdir(cwd)
    W1 = load_checkpoint(str(wd / "logs" / "model_final.pth"))
    W0 = synthetic_weights(EngineSpec(num_classes=2), seed=0)
    k = STEM + ".weight"
    assert W1[k].shape == (64, 3, 7, 7) and set(W1) == set(W0)
    assert not np.array_equal(W1[k], W0[k]) and np.isfinite(W1[k]).all()
    assert not np.array_equal(W1["backbone.bottom_up.res2.0.conv1.weight"], W0["backbone.bottom_up.res2.0.conv1.weight"])
