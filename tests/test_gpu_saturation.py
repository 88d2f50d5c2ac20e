"""Saturation counting: elements a stage clamps to the fp16 range are counted per stage, and nothing else changes.

* operators: exact counts of rs_op_conv2d (conv_igemm, conv_deep, deconv), rs_op_conv2d_split, rs_op_bneck_tail and rs_op_bneck_tail_split against a float64
  NumPy count on integer-valued data whose outputs are either |x| <= 30 000 or >= 100 000 (so fp16 rounding of an intermediate never
  moves a value across the 65 504 bound); outputs with the counter set are bit-identical to outputs without it;
* engine: exact preprocess counts, attribution to the stage whose bias was raised, no count on clean weights, graph replay against
  eager forwards, two lanes, and the Predictor's on_saturation modes.
GPU inputs stay finite except in the operator tests, where no address depends on a value."""
import ctypes as C
import os
import subprocess
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import (Engine, LanePipeline, Predictor, RsSaturationError, SaturationWarning, _check, load_library)
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import _ohwi, _perm_k64, synthetic_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = 65504.0


def _bad(v):
    return int(np.count_nonzero(~(np.abs(v) <= LIM)))


def _relu(v):
    return np.where(v > 0, v, 0.0)          # NaN -> 0, as the kernels' v > 0 ? v : 0


def _conv_ref(x, w, b, pad):
    """x (N,H,W,Cin) float64, w (Cout,Cin,k,k) -> (N,Ho,Wo,Cout) float64, stride 1."""
    n, h, wd, cin = x.shape
    cout, _, k, _ = w.shape
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, cin))
    xp[:, pad:pad + h, pad:pad + wd] = x
    ho, wo = h + 2 * pad - k + 1, wd + 2 * pad - k + 1
    out = np.zeros((n, ho, wo, cout)) + b
    for dy in range(k):
        for dx in range(k):
            out += np.einsum("nhwc,oc->nhwo", xp[:, dy:dy + ho, dx:dx + wo], w[:, :, dy, dx])
    return out


def _margin_ok(v):
    a = np.abs(v[~np.isnan(v)])
    return bool(np.all((a <= 30000) | (a >= 100000)))


class Counter:
    def __init__(self):
        self.lib = load_library()
        self.buf = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def __enter__(self):
        torch.cuda.synchronize()
        self.buf.zero_()
        torch.cuda.synchronize()
        self.lib.rs_op_set_saturation_counter(C.c_void_p(self.buf.data_ptr()))
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.lib.rs_op_set_saturation_counter(None)
        self.value = int(self.buf.cpu()[0])


def _halo(a, pad):
    n, h, w, c = a.shape
    o = np.zeros((n, h + 2 * pad, w + 2 * pad, c), a.dtype)
    o[:, pad:pad + h, pad:pad + w] = a
    return o


def _conv_data(rng, n, h, w, cin, cout, k, nan=False):
    """Integer data: a few output channels get a bias of +-2e5 (clamped with and without ReLU), channel 0 of the input carries 0 / 400
    with weight 500 into output channels 8..15 (per-pixel saturation), the rest small integers."""
    x = rng.integers(-2, 3, size=(n, h, w, cin)).astype(np.float64)
    x[..., 0] = rng.choice([0.0, 400.0], size=(n, h, w))
    wt = rng.integers(-1, 2, size=(cout, cin, k, k)).astype(np.float64)
    wt[:, 0] = 0.0
    wt[8:16, 0, k // 2, k // 2] = 500.0
    b = np.zeros(cout)
    b[:4] = 2e5
    b[4:8] = -2e5
    if nan:
        x[0, h // 2, w // 2, 1] = np.nan
    return x, wt, b


def _run_conv(x, wt, b, pad, relu, variant, deconv=False, split=False):
    lib = load_library()
    dev = torch.device("cuda:0")
    n, h, w, cin = x.shape
    if deconv:                                   # wt: (Cin, Cout, 2, 2) ConvTranspose2d weight -> rows (dy, dx, co) x ci
        cout = wt.shape[1]
        g = wt.transpose(2, 3, 1, 0).reshape(4 * cout, cin)
        wp = _ohwi(g[:, :, None, None].astype(np.float32), cin)
        bias = np.tile(b.astype(np.float32), 4)
        k = 1
        oh, ow = 2 * h, 2 * w
    else:
        cout, k = wt.shape[0], wt.shape[2]
        wp = _ohwi(wt.astype(np.float32), cin)
        bias = b.astype(np.float32)
        oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    xh = _halo(x.astype(np.float16), max(pad, 1))
    in_halo = max(pad, 1)
    if split:                                   # integer data: hi = value, lo = 0; weight scales 1
        xh = np.concatenate([xh.reshape(-1), np.zeros(xh.size, np.float16)])
        wp2 = np.concatenate([wp.reshape(-1), np.zeros(wp.size, np.float16)])
    xd = torch.from_numpy(np.ascontiguousarray(xh)).to(dev)
    wd = torch.from_numpy(np.ascontiguousarray(wp2 if split else wp)).to(dev)
    bd = torch.from_numpy(bias).to(dev)
    osz = n * oh * ow * cout
    od = torch.zeros(osz * (2 if split else 1), dtype=torch.float16, device=dev)
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())
    if split:
        sd = torch.ones(wp.shape[0], dtype=torch.float32, device=dev)
        rc = lib.rs_op_conv2d_split(P(xd), xh.size // 2, P(wd), wp.size, P(sd), P(bd), P(od), osz, None, 0, None, 0,
                                    n, h, w, cin, in_halo, k, k, 1, pad, cout, wp.shape[1], 0, int(relu), 0, int(deconv), variant, None)
    else:
        rc = lib.rs_op_conv2d(P(xd), P(wd), P(bd), P(od), None, None, n, h, w, cin, in_halo, k, k, 1, pad, cout, wp.shape[1], 0,
                              int(relu), 0, int(deconv), variant, 1, None)
    _check(lib, rc, "rs_op_conv2d")
    torch.cuda.synchronize()
    return od.cpu().numpy().view(np.uint16).copy()


def _deconv_ref(x, wt, b):
    n, h, w, cin = x.shape
    cout = wt.shape[1]
    out = np.zeros((n, 2 * h, 2 * w, cout))
    for dy in range(2):
        for dx in range(2):
            out[:, dy::2, dx::2] = np.einsum("nhwc,co->nhwo", x, wt[:, :, dy, dx]) + b
    return out


@pytest.mark.parametrize("case", ["igemm3x3", "igemm3x3_relu", "deep12", "deep12_relu", "deconv_relu", "deconv", "split_igemm", "split_deep12_relu",
                                  "igemm_nan", "igemm_nan_relu", "wreg", "wreg_relu", "wreg_nan"])
def test_conv_operator_counts_exactly(gpu_required, case):
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    relu = case.endswith("relu")
    nan = "nan" in case
    deconv = case.startswith("deconv")
    k = 3
    if case.startswith("deep") or case.startswith("split_deep"):
        variant, cin, cout, n, h, w = 12, 64, 256, 2, 19, 23
    elif case.startswith("wreg"):                # conv_wreg.hip (variant 22): 1x1, Cin 256, a NaN is stored as -65504 and counted
        variant, cin, cout, n, h, w, k = 22, 256, 256, 3, 21, 25, 1
    elif deconv:
        variant, cin, cout, n, h, w = -1, 64, 128, 3, 7, 7
    else:
        variant, cin, cout, n, h, w = 0, 64, 128, 2, 13, 17
    if deconv:
        x, wt, b = _conv_data(rng, n, h, w, cin, cout, 1)
        wt = np.ascontiguousarray(wt[:, :, 0, 0].T[:, :, None, None].repeat(2, 2).repeat(2, 3))   # (Cin, Cout, 2, 2)
        wt[0] = 0.0
        wt[0, 8:16] = 500.0
        ref = _deconv_ref(x, wt, b)
    else:
        x, wt, b = _conv_data(rng, n, h, w, cin, cout, k, nan=nan)
        ref = _conv_ref(x, wt, b, k // 2)
    if relu:
        ref = _relu(ref)
    assert _margin_ok(ref)
    want = _bad(ref)
    assert want > 0
    split = case.startswith("split")
    pad = 0 if deconv else k // 2
    plain = _run_conv(x, wt, b, pad, relu, variant, deconv=deconv, split=split)
    with Counter() as c:
        got = _run_conv(x, wt, b, pad, relu, variant, deconv=deconv, split=split)
    assert c.value == want, (case, c.value, want)
    assert np.array_equal(plain, got), "outputs changed with the counter set"


@pytest.mark.parametrize("split,width,proj,with_next", [(False, 64, False, True), (False, 128, False, True), (False, 64, True, True), (False, 128, False, False),
                                                          (True, 64, False, True), (True, 128, False, True), (True, 64, True, True), (True, 128, False, False)])
def test_bneck_tail_counts_all_three_clamp_points(gpu_required, split, width, proj, with_next):
    """rs_op_bneck_tail (fp16) and rs_op_bneck_tail_split: conv2 output, block output and next conv1 output all count, identity and projection
    shortcut.  Integer data: every lo plane is 0 and every row scale 1."""
    lib = load_library()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(width + 7 * proj + 13 * with_next + 29 * split)
    n, h, w = 2, 11, 13
    cb, c4 = width, 4 * width
    t1 = rng.integers(0, 2, size=(n, h, w, cb)).astype(np.float64)
    xin = rng.integers(0, 3, size=(n, h, w, 64 if proj else c4)).astype(np.float64)
    w2 = rng.integers(-1, 2, size=(cb, cb, 3, 3)).astype(np.float64)
    b2 = np.zeros(cb); b2[:2] = 2e5                      # conv2: two saturated channels
    w3 = rng.integers(-1, 2, size=(c4, cb, 1, 1)).astype(np.float64)
    w3[:, :2] = 0.0
    w3[:6, 0] = 2.0                                      # block output: six channels fed by a saturated conv2 channel
    b3 = np.zeros(c4)
    wsc = rng.integers(-1, 2, size=(c4, 64, 1, 1)).astype(np.float64)
    w1 = rng.integers(-1, 2, size=(cb, c4, 1, 1)).astype(np.float64)
    w1[:, :6] = 0.0
    w1[:3, 0] = 2.0                                      # next conv1: three channels fed by a saturated block output channel
    b1 = np.zeros(cb)
    t2 = _relu(_conv_ref(t1, w2, b2, 1))
    assert _margin_ok(t2)
    cnt = _bad(t2)
    t2 = np.minimum(t2, LIM)
    out = _relu(_conv_ref(t2, w3, b3, 0) + (_conv_ref(xin, wsc, np.zeros(c4), 0) if proj else xin))
    assert _margin_ok(out)
    cnt += _bad(out)
    out = np.minimum(out, LIM)
    if with_next:
        t1n = _relu(_conv_ref(out, w1, b1, 0))
        assert _margin_ok(t1n)
        cnt += _bad(t1n)
    assert cnt > 0

    def planes(a):                                       # fp16 tensor; split: the hi plane, then a zero lo plane
        a = np.ascontiguousarray(a, np.float16).reshape(-1)
        return torch.from_numpy(np.concatenate([a, np.zeros_like(a)]) if split else a).to(dev), a.size

    (t1d, t1_lo), (xd, x_lo) = planes(_halo(t1.astype(np.float16), 1)), planes(_halo(xin.astype(np.float16), 1))
    w2d, _ = planes(_ohwi(w2.astype(np.float32), cb))
    w3k = _perm_k64(_ohwi(w3.astype(np.float32), cb), cb)
    wsck = _ohwi(wsc.astype(np.float32), 64)
    w3d, _ = planes(np.concatenate([w3k, wsck], axis=1) if (split and proj) else w3k)     # split projection form: [conv3 | shortcut] per row
    wscd, _ = planes(wsck)
    w1d, _ = planes(_perm_k64(_ohwi(w1.astype(np.float32), c4), 64))
    b2d, b3d, b1d = (torch.from_numpy(v.astype(np.float32)).to(dev) for v in (b2, b3, b1))
    s2d, s3d, s1d = (torch.ones(k, dtype=torch.float32, device=dev) for k in (cb, c4, cb))
    P = lambda t: C.c_void_p(t.data_ptr())
    out_lo, t1n_lo = n * (h + 2) * (w + 2) * c4, n * (h + 2) * (w + 2) * cb
    nx = lambda t: P(t) if with_next else None

    def run():
        outd = torch.zeros(out_lo * (2 if split else 1), dtype=torch.float16, device=dev)
        t1nd = torch.zeros(t1n_lo * (2 if split else 1), dtype=torch.float16, device=dev)
        torch.cuda.synchronize()
        if split:
            rc = lib.rs_op_bneck_tail_split(P(t1d), t1_lo, P(w2d), P(s2d), P(b2d), P(w3d), P(s3d), P(b3d), None if proj else P(xd), x_lo, P(outd), out_lo,
                                            nx(w1d), nx(s1d), nx(b1d), nx(t1nd), t1n_lo, P(xd) if proj else None, x_lo, n, h, w, width, None)
        else:
            rc = lib.rs_op_bneck_tail(P(t1d), P(w2d), P(b2d), P(w3d), P(b3d), None if proj else P(xd), P(outd), nx(w1d), nx(b1d), nx(t1nd),
                                      P(xd) if proj else None, P(wscd) if proj else None, n, h, w, width, None)
        _check(lib, rc, "rs_op_bneck_tail")
        torch.cuda.synchronize()
        return outd.cpu().numpy().view(np.uint16).copy(), t1nd.cpu().numpy().view(np.uint16).copy()

    plain = run()
    with Counter() as c:
        got = run()
    assert c.value == cnt, (c.value, cnt)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])


# ------------------------------------------------------------------------------------------------------------------ engine
SMALL = dict(num_classes=2, min_size_test=192, max_size_test=320, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200)


def _spec_sat(**kw):
    base = EngineSpec(**SMALL)
    std = tuple((255.0 - m) / 65512.0 for m in base.pixel_mean)
    return base.replace(pixel_std=std, **kw)


def _tile(v, n=1):
    return np.full((n, 128, 128, 3), v, np.uint8)


@pytest.mark.parametrize("mode", ["fp16", "split", "fp32"])
def test_preprocess_count_is_exact_and_per_forward(gpu_required, mode):
    spec = _spec_sat(precision=mode)
    W = synthetic_weights(spec, seed=0)
    eng = Engine(spec, W, (128, 128, 3), max_batch=4)
    try:
        rh, rw, _, _ = eng.net_shape()
        full = rh * rw * 3
        A, B = _tile(255), _tile(110)
        for n in (1, 4):
            for t, k in ((A, 1), (B, 0), (A, 1), (B, 0)):
                eng.infer(np.repeat(t, n, axis=0))
                sat = eng.saturation()
                want = 0 if mode == "fp32" else k * n * full
                assert sat.get("preprocess", 0) == want, (mode, n, k, sat)
                if mode == "fp32":
                    assert sat == {}
        mixed = np.concatenate([A, B, A, B])
        eng.infer(mixed)
        assert eng.saturation().get("preprocess", 0) == (0 if mode == "fp32" else 2 * full)
    finally:
        eng.close()


def _raised_weights(spec, layer="backbone.bottom_up.res4.0.conv3", ch=5):
    W = synthetic_weights(spec, seed=0)
    W = dict(W)
    b = W[layer + ".norm.bias"].copy()
    b[ch] += 1e5
    W[layer + ".norm.bias"] = b
    return W


@pytest.mark.parametrize("mode", ["fp16", "split"])
def test_attribution_to_the_raised_stage(gpu_required, mode):
    spec = EngineSpec(**SMALL).replace(precision=mode)
    eng = Engine(spec, _raised_weights(spec), (128, 128, 3), max_batch=2)
    try:
        n = 2
        eng.infer(np.stack([np.random.default_rng(i).integers(0, 256, (128, 128, 3), dtype=np.uint8) for i in range(n)]))
        sat = eng.saturation()
        names = [s["name"] for s in eng.stage_times()]
        hw = eng.tensor("res4", n=n).shape[1:3]
        st = "res4.0.conv3"
        assert st in names, names
        assert sat.get(st, 0) == n * hw[0] * hw[1], (sat, hw)
        for nm in names[:names.index(st)]:
            assert sat.get(nm, 0) == 0, (nm, sat)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["fp16", "split", "fp32"])
def test_no_counts_on_clean_weights(gpu_required, mode):
    from proj_roadsurf_amd.synthetic import synthetic_tiles
    spec = EngineSpec(num_classes=2).replace(precision=mode)
    eng = Engine(spec, synthetic_weights(spec, seed=0), (256, 256, 3), max_batch=16)
    try:
        eng.infer(synthetic_tiles(16, 256, 256, 3, seed=3))
        assert eng.saturation() == {}
    finally:
        eng.close()


def _stem_ref(x, w, b):
    """7x7 stride-2 pad-3 convolution of x (N,H,W,3) float64 with w (64,3,7,7), + b, ReLU."""
    n, hh, ww, _ = x.shape
    xp = np.zeros((n, hh + 6, ww + 6, 3))
    xp[:, 3:3 + hh, 3:3 + ww] = x
    ho, wo = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
    v = np.zeros((n, ho, wo, w.shape[0])) + b
    for dy in range(7):
        for dx in range(7):
            v += np.einsum("nhwc,oc->nhwo", xp[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2], w[:, :, dy, dx].astype(np.float64))
    return _relu(v)


@pytest.mark.parametrize("mode", ["fp16", "split"])
def test_fused_stem_counts_every_conv_pixel_once(gpu_required, mode):
    """The fused stem (stem_fused.hip) computes overlapping 17x17 conv patches per 8x8 pooled patch; each conv pixel must count once.  The stem
    weights are scaled so that about three quarters of the positive conv values exceed 65504; reference: the convolution of the engine's own net
    input with the folded weights in float64.  Values within 0.5 % of the bound are left to either side (fp16 weight rounding); a patch row or
    column counted twice or not at all moves the count by about 10 %."""
    from proj_roadsurf_amd.weights import _fold_bn
    from tests.util import synthetic_tiles
    spec = EngineSpec(**SMALL).replace(min_size_test=192, precision=mode)
    W = dict(synthetic_weights(spec, seed=0))
    tiles = synthetic_tiles(2, 192, 192, 3, seed=11)             # 192 x 192: no resize
    name = "backbone.bottom_up.stem.conv1"
    w1, b1 = _fold_bn(W, name, spec.bn_eps)
    approx = tiles.astype(np.float64) - np.array(spec.pixel_mean)
    cc = np.concatenate([_stem_ref(approx[..., ::o], w1, np.zeros_like(b1)).reshape(-1) for o in (1, -1)])
    F = float(LIM / np.percentile(cc[cc > 0], 25))
    W[name + ".weight"] = W[name + ".weight"] * np.float32(F)
    eng = Engine(spec, W, (192, 192, 3), max_batch=2)
    try:
        eng.infer(tiles)
        sat = eng.saturation()
        x = eng.tensor("net_input", n=2).astype(np.float64)[..., :3]          # model channel order; hi + lo in split
    finally:
        eng.close()
    w, b = _fold_bn(W, name, spec.bn_eps)
    v = _stem_ref(x, w, b)
    lo_cnt, hi_cnt = int((v > LIM * 1.005).sum()), int((v > LIM * 0.995).sum())
    assert lo_cnt > 100000
    got = sat.get("stem.conv1+maxpool", 0)
    assert lo_cnt <= got <= hi_cnt, (got, lo_cnt, hi_cnt)
    assert hi_cnt - lo_cnt < 0.03 * lo_cnt, (lo_cnt, hi_cnt)


@pytest.mark.parametrize("mode", ["fp16", "split", "fp32"])
def test_no_counts_on_the_golden_fixture(gpu_required, mode):
    from tests.golden.make_golden import SPEC_KW
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_small.npz"))
    spec = EngineSpec(**SPEC_KW).replace(precision=mode)
    tiles = np.resize(g["tiles"], (16,) + g["tiles"].shape[1:])
    eng = Engine(spec, synthetic_weights(EngineSpec(**SPEC_KW), 0), tiles.shape[1:], max_batch=16)
    try:
        eng.infer(tiles)
        assert eng.saturation() == {}
    finally:
        eng.close()


def test_no_counts_on_a_trained_like_detector(gpu_required):
    from proj_roadsurf_amd.synthetic import synthetic_scenes, train_trained_like
    spec = EngineSpec(num_classes=2)
    W, curve = train_trained_like(spec, 256, steps=300, seed=0)
    tiles = synthetic_scenes(16, 256, 256, 3, seed=424242, objects=(4, 12))[0]
    for mode in ("fp16", "split", "fp32"):
        eng = Engine(spec.replace(precision=mode), W, (256, 256, 3), max_batch=16)
        try:
            eng.infer(tiles)
            assert eng.saturation() == {}, (mode, eng.saturation())
        finally:
            eng.close()


_CHILD = r"""
import json, sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_saturation import _spec_sat, _tile
from proj_roadsurf_amd.engine import Engine
from proj_roadsurf_amd.weights import synthetic_weights
spec = _spec_sat(precision=sys.argv[2])
eng = Engine(spec, synthetic_weights(spec, seed=0), (128, 128, 3), max_batch=1)
out = []
for v in (255, 110, 255, 110):
    d = eng.infer(_tile(v))[0]
    out.append({"sat": eng.saturation(), "boxes": d.pred_boxes.tolist(), "scores": d.scores.tolist(), "classes": d.pred_classes.tolist()})
eng.close()
print("RESULT" + json.dumps(out))
"""


@pytest.mark.parametrize("mode", ["fp16", "split"])
def test_graph_replay_counts_like_eager(gpu_required, mode):
    res = {}
    for g in ("1", "0"):
        env = dict(os.environ, RS_GRAPH_SMALL=g)
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, mode], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][0]
        import json
        res[g] = json.loads(line[6:])
    assert res["1"] == res["0"]
    assert res["1"][0]["sat"].get("preprocess", 0) > 0 and res["1"][1]["sat"].get("preprocess", 0) == 0


@pytest.mark.parametrize("shared", [False, True])
def test_two_lanes_report_each_batch(gpu_required, shared):
    spec = _spec_sat(precision="fp16")
    pipe = LanePipeline(spec, synthetic_weights(spec, seed=0), (128, 128, 3), max_batch=2, lanes=2, shared_stream=shared)
    try:
        rh, rw, _, _ = pipe.engines[0].net_shape()
        kinds = [1, 0, 0, 1, 1, 1, 0, 1, 0, 0]
        batches = [_tile(255 if k else 110, 2) for k in kinds]
        got = [pipe.last_saturation.get("preprocess", 0) for _ in pipe.run(iter(batches))]
        assert got == [k * 2 * rh * rw * 3 for k in kinds]
    finally:
        pipe.close()


def test_predictor_on_saturation_modes(gpu_required):
    spec = _spec_sat(precision="fp16")
    W = synthetic_weights(spec, seed=0)
    ims = [_tile(255)[0], _tile(110)[0], _tile(110)[0]]
    p = Predictor(spec, W, max_batch=2, lanes=2)
    try:
        with pytest.warns(SaturationWarning):
            p.predict_batch(ims)
        with warnings.catch_warnings():
            warnings.simplefilter("error", SaturationWarning)
            p.predict_batch(ims[1:])                      # clean batch: no warning
            assert p.last_saturation == {}
        with pytest.warns(SaturationWarning):
            p(ims[0])
        p.on_saturation = "raise"
        with pytest.raises(RsSaturationError):
            p(ims[0])
        with pytest.raises(RsSaturationError):
            list(p.predict_stream(iter([ims[:2], ims[1:]])))
        p.on_saturation = "ignore"
        with warnings.catch_warnings():
            warnings.simplefilter("error", SaturationWarning)
            out = list(p.predict_stream(iter([ims[:2], ims[1:]])))
        assert len(out) == 2 and p.last_saturation == {}
    finally:
        p.close()


def test_make_detections_logs_saturation_once_per_dataset(gpu_required, tmp_path, caplog):
    """A YAML whose MODEL.PIXEL_STD is far below 1 saturates the pre-processing of the synthetic tiles: the CLI logs one warning line for the dataset
    (affected batches, first tile, largest stages) and still exits 0; the same job with the default PIXEL_STD logs none."""
    import logging
    import yaml
    from proj_roadsurf_amd import make_detections
    from tests.test_vector_cli import _cli_dataset
    cfg, wd = _cli_dataset(tmp_path, 5)
    cwd = os.getcwd()
    d2_path = tmp_path / "d2.yaml"
    try:
        caplog.set_level(logging.WARNING, logger="make_detections")
        assert make_detections.main([cfg, "--synthetic-weights", "--batch", "2", "--tagged-samples", "0", "--precision", "fp16"]) == 0
        os.chdir(cwd)
        assert not [r for r in caplog.records if "clamped to the fp16 range" in r.getMessage()]
        d2 = yaml.safe_load(open(d2_path))
        d2["MODEL"]["PIXEL_STD"] = [0.001, 0.001, 0.001]
        yaml.safe_dump(d2, open(d2_path, "w"))
        caplog.clear()
        assert make_detections.main([cfg, "--synthetic-weights", "--batch", "2", "--tagged-samples", "0", "--precision", "fp16"]) == 0
    finally:
        os.chdir(cwd)
    lines = [r.getMessage() for r in caplog.records if "clamped to the fp16 range" in r.getMessage()]
    assert len(lines) == 1, lines
    assert lines[0].startswith("val: 3 batch(es)") and "18_100_200.tif" in lines[0] and "preprocess" in lines[0], lines[0]
