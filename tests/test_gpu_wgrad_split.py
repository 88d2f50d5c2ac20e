"""Weight gradients of the fp32 trainer on split operands (csrc/conv_wgrad.hip conv_wgrad_split_kernel, rs_op_conv2d_wgrad_split,
rs_trainer_set_wgrad_mode, ``Trainer(wgrad="split")``, ``train_model.py --wgrad split``) on the GPU.

The operator is held, per element, to the derived bound of tests/wgrad_split_ref.py plus the accumulation-order error of the fp32 kernel,
which is measured inside the test from rs_op_conv2d_wgrad_f32 on the same inputs:

    |got - ref64| <= 2^-20 S + 2^-36 M max|dy| max|x| + E_f32"""
import ctypes as C
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd.engine import RsError, Trainer, _check, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests.util import synthetic_tiles
from tests import wgrad_split_ref as R

pytestmark = pytest.mark.gpu

CONV_CASES = [                              # the cases of test_conv_wgrad_f32_matches_autograd
    (256, 256, 3, 1, (25, 27), 2, 0),
    (64, 128, 1, 1, (19, 23), 3, 1),
    (256, 128, 1, 2, (26, 30), 2, 0),
    (128, 128, 3, 1, (14, 14), 5, 3),
    (512, 16, 1, 1, (13, 13), 2, 0),
]
RANGE_CASE = (128, 128, 3, 1, (14, 14), 5, 3)


def _halo(x_nhwc: torch.Tensor, pad: int) -> torch.Tensor:
    n, h, w, c = x_nhwc.shape
    out = torch.zeros((n, h + 2 * pad, w + 2 * pad, c), dtype=x_nhwc.dtype)
    out[:, pad:pad + h, pad:pad + w] = x_nhwc
    return out


def run(entry, x, dy, k, stride, pad, scale=None, splits=0, in_halo=None, dy_halo=1):
    """x (N,Cin,H,W), dy (N,Cout,Ho,Wo) fp32 -> dW (Cout,Cin,k,k) fp32 from operator ``entry``; the output starts as NaN."""
    lib = load_library()
    dev = torch.device("cuda:0")
    n, cin, hi, wi = x.shape
    cout = dy.shape[1]
    in_halo = pad if in_halo is None else in_halo
    xd = _halo(x.permute(0, 2, 3, 1).float().contiguous(), in_halo).to(dev)
    dyd = _halo(dy.permute(0, 2, 3, 1).float().contiguous(), dy_halo).to(dev)
    kpad = k * k * cin
    gd = torch.full((cout, kpad), float("nan"), dtype=torch.float32, device=dev)
    sd = scale.to(dev) if scale is not None else None
    torch.cuda.synchronize()
    rc = getattr(lib, entry)(C.c_void_p(dyd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(gd.data_ptr()),
                             C.c_void_p(sd.data_ptr()) if sd is not None else None,
                             n, hi, wi, cin, in_halo, k, k, stride, pad, cout, kpad, dy_halo, splits, None)
    _check(lib, rc, entry)
    torch.cuda.synchronize()
    return gd.cpu().reshape(cout, k, k, cin).permute(0, 3, 1, 2).contiguous().numpy()


def split(*a, **kw):
    return run("rs_op_conv2d_wgrad_split", *a, **kw)


def f32(*a, **kw):
    return run("rs_op_conv2d_wgrad_f32", *a, **kw)


def ref64(x, dy, k, stride, pad, scale=None):
    """(exact gradient, S = the same sum over |dy| |x|) in float64, scaled like the operator's result."""
    out = []
    for a, b in ((x.double(), dy.double()), (x.double().abs(), dy.double().abs())):
        w = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(a, w, stride=stride, padding=pad).backward(b)
        g = w.grad.detach()
        out.append((g * scale.double()[:, None, None, None] if scale is not None else g).numpy())
    return out


def limit(x, dy, S, e_f32, scale=None):
    m_terms = dy.shape[0] * dy.shape[2] * dy.shape[3]
    finite = lambda t: t[torch.isfinite(t)]
    second = R.bound(0.0, m_terms, float(finite(dy).abs().max()), float(finite(x).abs().max()))
    if scale is not None:
        second = second * scale.double().numpy()[:, None, None, None]
    return 2.0 ** -20 * S + second + e_f32


def conv_inputs(case, family="gaussian"):
    cin, cout, k, stride, (h, w), n, splits = case
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    rng = np.random.default_rng(cin + cout + k + 1)
    dy, x = R.family(family, rng, (n, cout, ho, wo), (n, cin, h, w))
    scale = torch.as_tensor(rng.random(cout).astype(np.float32) + 0.5) if k == 3 else None
    return torch.as_tensor(x), torch.as_tensor(dy), k, stride, pad, scale, splits


def check_inside_bound(x, dy, k, stride, pad, scale, splits, tag, **halos):
    ref, S = ref64(x, dy, k, stride, pad, scale)
    e_f32 = float(np.abs(f32(x, dy, k, stride, pad, scale=scale, splits=splits, **halos) - ref).max())
    got = split(x, dy, k, stride, pad, scale=scale, splits=splits, **halos)
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} elements not written or not finite"
    err = np.abs(got - ref)
    lim = limit(x, dy, S, e_f32, scale)
    print(f"{tag}: max err {err.max():.3e} (fp32 kernel {e_f32:.3e}), largest err / bound {float((err / lim).max()):.3f}")
    assert (err <= lim).all(), (tag, float((err / lim).max()))
    return got


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_operator_against_float64(gpu_required, case):
    x, dy, k, stride, pad, scale, splits = conv_inputs(case)
    check_inside_bound(x, dy, k, stride, pad, scale, splits, str(case), in_halo=max(pad, 1))


def test_operator_fc_shape_with_scale(gpu_required):
    """Linear layer as a 1x1 convolution over an (M x 1) image, FrozenBN-style per-channel scale (test_conv_wgrad_scale_and_fc_shape)."""
    g = torch.Generator().manual_seed(3)
    m, kin, nout = 333, 1024, 256
    a = torch.randn(m, kin, generator=g)
    dy = torch.randn(m, nout, generator=g) * 0.05
    scale = torch.rand(nout, generator=g) + 0.5
    check_inside_bound(a.t().reshape(1, kin, m, 1), dy.t().reshape(1, nout, m, 1), 1, 1, 0, scale, 0, "fc 333 x 1024 -> 256", in_halo=0, dy_halo=0)


@pytest.fixture(scope="module")
def range_base():
    x, dy, k, stride, pad, scale, splits = conv_inputs(RANGE_CASE)
    return x, dy, k, stride, pad, scale, splits, split(x, dy, k, stride, pad, scale=scale, splits=splits, in_halo=1)


@pytest.mark.parametrize("e_dy,e_x", [(-30, 10), (12, -20)])
def test_power_of_two_factors_pass_through_bit_for_bit(gpu_required, range_base, e_dy, e_x):
    x, dy, k, stride, pad, scale, splits, base = range_base
    got = split(torch.ldexp(x, torch.tensor(e_x)), torch.ldexp(dy, torch.tensor(e_dy)), k, stride, pad, scale=scale, splits=splits, in_halo=1)
    want = np.ldexp(base, e_dy + e_x).astype(np.float32)
    assert float(np.abs(want[want != 0]).min()) >= 2.0 ** -126      # no result left the normal range: the factor is exact on every one
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_zero_gradient_gives_exact_zeros(gpu_required, range_base):
    x, dy, k, stride, pad, scale, splits, _ = range_base
    got = split(x, torch.zeros_like(dy), k, stride, pad, scale=scale, splits=splits, in_halo=1)
    assert np.array_equal(got.view(np.uint32), np.zeros_like(got).view(np.uint32))


def test_heavy_tailed_gradient_stays_inside_the_bound(gpu_required):
    x, dy, k, stride, pad, scale, splits = conv_inputs(RANGE_CASE, "heavy_tail")
    check_inside_bound(x, dy, k, stride, pad, scale, splits, "heavy tail", in_halo=1)


def test_one_nan_reaches_its_output_channel_only(gpu_required, range_base):
    x, dy, k, stride, pad, scale, splits, _ = range_base
    bad = dy.clone()
    bad[3, 7, 5, 9] = float("nan")
    got = split(x, bad, k, stride, pad, scale=scale, splits=splits, in_halo=1)
    assert not np.isfinite(got[7]).any()
    assert np.isfinite(np.delete(got, 7, axis=0)).all()


def test_two_calls_give_the_same_bits_and_every_split_count_holds(gpu_required, range_base):
    x, dy, k, stride, pad, scale, splits, base = range_base
    again = split(x, dy, k, stride, pad, scale=scale, splits=splits, in_halo=1)
    assert np.array_equal(again.view(np.uint32), base.view(np.uint32))
    for s in (1, 3):
        check_inside_bound(x, dy, k, stride, pad, scale, s, f"splits {s}", in_halo=1)


# ---------------------------------------------------------------------------------------------------------------- the assembled step
# relative L2 distance between a weight gradient of the split mode and of the fp32 mode: 4x the worst value measured on an MI355X, and in
# no case above 1e-5 (one hundredth of the autograd bar).  Measured over the 66 weight-gradient tensors (profiles/wgrad_split/README.md,
# test_gpu_wgrad_split.txt): 6.18e-8 (rpn_head.heads) .. 1.633e-7 (res5.0.conv1), res5 around 1.6e-7, res3 / res4 around 1.0e-7: the fp16
# pair's 2^-22 representation, averaged.
MEASURED_WORST_MODE_DISTANCE = 1.633e-7
MODE_DISTANCE_CAP = 1e-5


def test_assembled_step_in_both_modes(gpu_required):
    """The setting of test_reference_precision_training_step_matches_autograd (256 x 256 tiles, batch 2, sampling 256 / 0.5 / 64 / 0.25, seed 5)
    on ONE fp32 trainer: the step in mode f32, in mode split, split again, f32 again.  Nothing but the weight-gradient product changes, so
    the five losses and every bias gradient are bit-identical between the modes; every weight gradient of the split mode is within 1e-3
    relative L2 of autograd (the existing bar), its rows beyond the real predictor rows are exactly 0, a second split step repeats the
    first one's bits and the f32 step comes back bit for bit.  The distance between the modes is printed per tensor; measured on an
    MI355X (profiles/wgrad_split/README.md): at most 1.633e-7 relative L2 (res5.0.conv1), at least 6.18e-8 (the RPN heads); the bound is 4x
    the worst, 6.53e-7.  Against autograd the split mode's worst tensor is 4.62e-4 (res5.2.conv1)."""
    from oracle import train_oracle as T
    from tests.test_gpu_trainer import _d2_grad, _engine_step, _oracle_losses_on_engine_samples, _two_image_problem, trainable_layers
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision="fp32")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _two_image_problem()
    layers = list(trainable_layers(spec))
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=1.0)

    def step(mode):
        tr.set_wgrad_mode(mode)
        targets, where = _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=5)
        out = {"losses": tr.tensor("losses")[:5].copy()}
        for layer in layers:
            out[f"g:{layer}.w"] = tr.tensor(f"g:{layer}.w").copy()
            try:
                out[f"g:{layer}.b"] = tr.tensor(f"g:{layer}.b").copy()
            except RsError:
                pass                                  # FrozenBN layers have no trainable bias
        return out, targets, where

    same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        a, _, _ = step("f32")
        b, targets, where = step("split")
        assert tr.wgrad == "split"
        assert same(a["losses"], b["losses"]), (a["losses"], b["losses"])
        biases = [n for n in a if n.endswith(".b")]
        assert len(biases) >= 10
        for n in biases:
            assert same(a[n], b[n]), n
        W = {k2: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k2, v in Wn.items()}
        for k2 in T.trainable_keys(W):
            W[k2].requires_grad_(True)
        _, ref = _oracle_losses_on_engine_samples(tr, spec, W, gt_boxes, polys, targets, where)
        sum(ref[n] for n in ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")).backward()
        worst, dist = {}, {}
        for layer in layers:
            want, got = _d2_grad(W, layer, spec), b[f"g:{layer}.w"]
            assert got.shape == want.shape, (layer, got.shape, want.shape)
            worst[layer] = float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
            dist[layer] = float(np.linalg.norm(got.astype(np.float64) - a[f"g:{layer}.w"]) / max(np.linalg.norm(a[f"g:{layer}.w"]), 1e-30))
        for layer, rows in (("proposal_generator.rpn_head.heads", 5 * spec.num_anchors), ("roi_heads.box_predictor", 5 * spec.num_classes + 1),
                            ("roi_heads.mask_head.predictor16", spec.num_classes)):
            assert b[f"g:{layer}.w"].shape[0] > rows and not b[f"g:{layer}.w"][rows:].any(), layer
        for layer in sorted(dist, key=lambda n: -dist[n]):
            print(f"split vs f32 rel L2 {dist[layer]:.3e}   split vs autograd {worst[layer]:.3e}   {layer}")
        assert max(worst.values()) <= 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:6]
        bar = min(4 * MEASURED_WORST_MODE_DISTANCE, MODE_DISTANCE_CAP)
        assert max(dist.values()) <= bar, sorted(dist.items(), key=lambda kv: -kv[1])[:6]
        assert max(dist.values()) > 0.0, "the split mode ran the fp32 kernel"
        c, _, _ = step("split")
        for n in b:
            assert same(b[n], c[n]), f"second split step: {n}"
        d, _, _ = step("f32")
        for n in a:
            assert same(a[n], d[n]), f"back in mode f32: {n}"
    finally:
        tr.close()


def test_fp16_trainer_refuses_the_split_mode(gpu_required):
    spec = EngineSpec(num_classes=2, min_size_test=256, max_size_test=426)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=256.0)
    try:
        with pytest.raises(RsError, match="rs_trainer_set_wgrad_mode"):
            tr.set_wgrad_mode("split")
        assert tr.wgrad == "f32"
        tr.set_wgrad_mode("f32")
        assert tr.lib.rs_trainer_set_wgrad_mode(tr._h, 2) < 0
    finally:
        tr.close()


def test_train_model_cli_runs_in_split_mode(gpu_required, tmp_path, caplog):
    import json
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    cwd = os.getcwd()
    wd = _tiny_training_workdir(tmp_path)
    try:
        with pytest.raises(SystemExit, match="--wgrad split"):
            train_model.main([str(tmp_path / "config.yaml"), "--synthetic-weights", "--max-iter", "2", "--precision", "fp16", "--wgrad", "split",
                              "--tagged-samples", "0"])
        os.chdir(cwd)
        with caplog.at_level(logging.INFO, logger="train_model"):
            assert train_model.main([str(tmp_path / "config.yaml"), "--wgrad", "split", "--max-iter", "2", "--synthetic-weights", "--log-period", "1",
                                     "--tagged-samples", "0"]) == 0
    finally:
        os.chdir(cwd)
    assert any("wgrad: split" in r.getMessage() for r in caplog.records)
    lines = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
    assert [l["iteration"] for l in lines] == [0, 1]
    names = ("total_loss", "loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
    assert all(np.isfinite(l[k]) for l in lines for k in names), lines
