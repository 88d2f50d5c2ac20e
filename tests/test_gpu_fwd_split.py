"""Forward pass of the fp32 trainer on split operands (csrc/conv_igemm.hip TRAIN && SPLIT with the forward epilogue,
rs_op_conv2d_fwd_split, rs_trainer_set_fwd_mode, ``Trainer(fwd="split")``, ``train_model.py --fwd split``) on the GPU.

The operator is held, per element, to

    |y - y64| <= 2^-20 S + 2^-36 T max|x| rowmax|w| + E_f32 + 6 * 2^-24 (|gemm| + |bias| + sum |addend|),      S = sum |x||w|

with y64 from float64 numpy and E_f32 the largest error of the fp32 matrix-core kernel, rs_op_conv2d(use_glds = -1), on the same x and w
(zero bias, no addend), measured inside the test.  ReLU is 1-Lipschitz, so the bound carries through it.  Every case writes into a
NaN-filled output and runs every tile the dispatch can take for its row count, by number."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd.engine import MultiScaleTrainer, RsError, Trainer, _check, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests.util import synthetic_tiles
from tests import dgrad_split_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def tiles_for(cout):
    """The tile numbers a launch of `cout` rows can take (-1, the rule itself, runs too)."""
    return (-1, 2, 7, 14, 4) if cout % 256 == 0 else ((-1, 2, 7) if cout % 128 == 0 else (-1, 2))


def _halo(t_nhwc, pad, fill=0.0):
    n, h, w, c = t_nhwc.shape
    out = torch.full((n, h + 2 * pad, w + 2 * pad, c), fill, dtype=torch.float32)
    out[:, pad:pad + h, pad:pad + w] = t_nhwc
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Case:
    """x (n, cin, hi, wi), w (cout, k, k, cin) -- the engine's [cout][kpad] layout, kpad = k k cin -- bias (cout), optional res in y's
    (n, cout, ho, wo) shape and up in the coarser (n, cout, ceil(ho / 2), ceil(wo / 2)); everything fp32 torch."""

    def __init__(self, x, w, bias, k, stride, pad, res=None, up=None, relu=False, in_halo=1, out_halo=1, count=None):
        self.x, self.w, self.bias, self.k, self.stride, self.pad = x, w, bias, k, stride, pad
        self.res, self.up, self.relu, self.in_halo, self.out_halo, self.count = res, up, relu, in_halo, out_halo, count
        self.n, self.cin, self.hi, self.wi = x.shape
        self.cout = w.shape[0]
        self.kpad = k * k * self.cin
        self.ho, self.wo = (self.hi + 2 * pad - k) // stride + 1, (self.wi + 2 * pad - k) // stride + 1

    def replace(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    def gemm64(self, absolute=False):
        """(n, cout, ho, wo) float64: the exact product, or S, the same sum over magnitudes."""
        x, w = self.x.double(), self.w.double()
        if absolute:
            x, w = x.abs(), w.abs()
        return F.conv2d(x, w.permute(0, 3, 1, 2), stride=self.stride, padding=self.pad).numpy()

    def up_full(self):
        return None if self.up is None else self.up.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :self.ho, :self.wo]

    def _device_operands(self):
        nhwc = lambda t, p: None if t is None else _halo(t.permute(0, 2, 3, 1).float().contiguous(), p).to(DEV)
        return (nhwc(self.x, self.in_halo), self.w.reshape(self.cout, self.kpad).contiguous().to(DEV), self.bias.float().contiguous().to(DEV),
                nhwc(self.res, self.out_halo), nhwc(self.up, self.out_halo))

    def run_split(self, variant=-1, fill=NAN):
        """y (n, cout, ho, wo) fp32 from rs_op_conv2d_fwd_split; y starts as `fill` everywhere, halo included."""
        lib = load_library()
        xd, wd, bd, res, up = self._device_operands()
        h = self.out_halo
        yd = torch.full((self.n, self.ho + 2 * h, self.wo + 2 * h, self.cout), fill, dtype=torch.float32, device=DEV)
        cnt = torch.tensor([self.count], dtype=torch.int32, device=DEV) if self.count is not None else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        torch.cuda.synchronize()
        rc = lib.rs_op_conv2d_fwd_split(ptr(xd), ptr(wd), ptr(bd), ptr(yd), ptr(res), ptr(up), self.n, self.hi, self.wi, self.cin, self.in_halo,
                                        self.k, self.k, self.stride, self.pad, self.cout, self.kpad, h, int(self.relu), variant, ptr(cnt), None)
        _check(lib, rc, "rs_op_conv2d_fwd_split")
        torch.cuda.synchronize()
        full = yd.cpu()
        ring = torch.ones(full.shape[1:3], dtype=torch.bool)
        ring[h:h + self.ho, h:h + self.wo] = False
        self.last_halo_untouched = bool(torch.isnan(full[:, ring]).all()) if fill != fill else True
        return full[:, h:h + self.ho, h:h + self.wo].permute(0, 3, 1, 2).contiguous().numpy()

    def e_f32(self, ref):
        """Largest error of the fp32 matrix-core kernel on the same product (zero bias, no addend, no ReLU) against float64."""
        lib = load_library()
        xd, wd, _, _, _ = self._device_operands()
        h = self.out_halo
        out = torch.zeros((self.n, self.ho + 2 * h, self.wo + 2 * h, self.cout), dtype=torch.float32, device=DEV)
        bias = torch.zeros(self.cout + 64, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        rc = lib.rs_op_conv2d(C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(bias.data_ptr()), C.c_void_p(out.data_ptr()), None, None,
                              self.n, self.hi, self.wi, self.cin, self.in_halo, self.k, self.k, self.stride, self.pad, self.cout, self.kpad, h, 0, 1, 0, -1, -1, None)
        _check(lib, rc, "rs_op_conv2d (fp32)")
        torch.cuda.synchronize()
        got = out.cpu()[:, h:h + self.ho, h:h + self.wo].permute(0, 3, 1, 2).double().numpy()
        return float(np.abs(got - ref).max())


def make(name, n, hi, wi, cin, cout, k, stride=1, pad=None, in_halo=1, out_halo=1, seed=0, bias=True):
    pad = k // 2 if pad is None else pad
    rng = np.random.default_rng(2000 + seed)
    x, w = R.family(name, rng, (n, cin, hi, wi), (cout, k, k, cin))
    b = rng.standard_normal(cout).astype(np.float32) if bias else np.zeros(cout, np.float32)
    return Case(torch.as_tensor(x), torch.as_tensor(w), torch.as_tensor(b), k, stride, pad, in_halo=max(in_halo, pad), out_halo=out_halo)


def check_inside_bound(c, tag, variants=None):
    """Every tile of the case inside the per-element bound, on a NaN-filled y; returns the results by tile number."""
    ref, S = c.gemm64(), c.gemm64(absolute=True)
    e32 = c.e_f32(ref)
    fin = c.x[torch.isfinite(c.x)]
    lim = R.bound(S.transpose(0, 2, 3, 1).reshape(-1, c.cout), c.kpad, float(fin.abs().max()), c.w.reshape(c.cout, -1).abs().max(dim=1).values.numpy())
    lim = lim.reshape(c.n, c.ho, c.wo, c.cout).transpose(0, 3, 1, 2) + e32
    bias = c.bias.double().numpy()[None, :, None, None]
    adds = [a.double().numpy() for a in (c.res, c.up_full()) if a is not None]
    want = ref + bias + sum(adds)
    lim = lim + R.epilogue_allowance(ref, np.abs(bias) + sum(np.abs(a) for a in adds))
    if c.relu:
        want = np.maximum(want, 0.0)
    live = np.ones(want.shape, bool)
    if c.count is not None:
        live[c.count:] = False
    out = {}
    for v in variants or tiles_for(c.cout):
        got = c.run_split(v)
        assert c.last_halo_untouched, f"{tag} tile {v}: the halo of y was written"
        assert np.isnan(got[~live]).all(), f"{tag} tile {v}: an element outside the launch was written"
        assert np.isfinite(got[live]).all(), f"{tag} tile {v}: {int((~np.isfinite(got[live])).sum())} elements not written or not finite"
        if c.relu:
            assert (got[live] >= 0).all() and (got[live] == 0).any() and (got[live] > 0).any(), f"{tag} tile {v}: ReLU"
        err = np.abs(got.astype(np.float64) - want)[live]
        used = float((err / lim[live]).max())
        print(f"{tag} tile {v}: max err {err.max():.3e} (fp32 kernel {e32:.3e}), largest err / bound {used:.3f}")
        assert used <= 1.0, (tag, v, used)
        out[v] = got
    return out


@pytest.fixture(scope="module")
def base3x3():
    c = make("gaussian", 2, 14, 14, 64, 128, 3, seed=1)
    return c, c.run_split(-1)


@pytest.mark.parametrize("cout", [128, 256, 512])
def test_3x3_and_its_every_tile(gpu_required, cout):
    """64 -> 128 / 256 / 512 with T = 576 terms: the 16-row, 64 x 128, 128 x 256 and 256 x 256 tiles, forced, agree bit for bit."""
    c = make("gaussian", 2, 14, 14, 64, cout, 3, seed=1 if cout == 128 else cout)
    assert c.kpad >= 512
    got = check_inside_bound(c, f"3x3 64 -> {cout}")
    assert set(got) == set(tiles_for(cout)) and (cout < 256 or {7, 14, 4} <= set(got))
    for v, g in got.items():
        assert same_bits(g, got[-1]), f"tile {v} and the rule's tile differ"


def test_1x1(gpu_required):
    check_inside_bound(make("gaussian", 2, 14, 14, 256, 128, 1, seed=2), "1x1 256 -> 128")


@pytest.mark.parametrize("side", [14, 15])
def test_1x1_at_input_stride_2(gpu_required, side):
    """14 x 14 -> 7 x 7, and 15 x 15 -> 8 x 8 where the last tap sits on the last input pixel: the TRAIN && SPLIT loop with p.stride = 2."""
    c = make("gaussian", 2, side, side, 128, 256, 1, stride=2, seed=3 + side)
    assert (c.ho, c.wo) == ((side + 1) // 2,) * 2
    if side == 15:
        assert (c.ho - 1) * 2 == side - 1
    got = check_inside_bound(c, f"1x1 s2 {side} x {side} 128 -> 256")
    assert all(same_bits(g, got[-1]) for g in got.values())


def test_3x3_with_bias_res_and_relu(gpu_required, base3x3):
    c, _ = base3x3
    g = torch.Generator().manual_seed(11)
    check_inside_bound(c.replace(res=torch.randn((c.n, c.cout, c.ho, c.wo), generator=g), relu=True), "3x3 + bias + res + relu")


@pytest.mark.parametrize("relu", [False, True])
def test_1x1_with_up_from_the_coarser_map(gpu_required, relu):
    """The FPN top-down addend: every 2 x 2 output block reads one pixel of the 7 x 7 coarser map."""
    c = make("gaussian", 2, 14, 14, 256, 256, 1, seed=5)
    g = torch.Generator().manual_seed(12)
    up = torch.randn((2, 256, 7, 7), generator=g)
    got = check_inside_bound(c.replace(up=up, relu=relu), f"1x1 + up, relu {relu}")
    if not relu:      # the addend alone, exactly: zero x leaves bias + up
        z = c.replace(x=torch.zeros_like(c.x), up=up).run_split(-1)
        want = (c.bias.numpy()[None, :, None, None] + up.repeat_interleave(2, 2).repeat_interleave(2, 3).numpy()).astype(np.float32)
        assert same_bits(z, want)
    assert all(same_bits(g2, got[-1]) for g2 in got.values())


def test_fc_as_an_m_by_1_image(gpu_required):
    check_inside_bound(make("gaussian", 1, 70, 1, 1024, 256, 1, in_halo=0, out_halo=0, seed=6).replace(relu=True), "fc 70 x 1024 -> 256")


def test_16_row_head(gpu_required):
    got = check_inside_bound(make("gaussian", 2, 14, 14, 256, 16, 1, out_halo=0, seed=7), "head 256 -> 16")
    assert set(got) == {-1, 2}


def test_count_bounded_launch_writes_its_images_only(gpu_required):
    c = make("gaussian", 3, 9, 11, 128, 128, 3, seed=8)
    check_inside_bound(c.replace(count=2), "3x3 128 -> 128, 2 of 3 images")       # the third image's NaN fill survives
    pattern = c.replace(count=2).run_split(-1, fill=-1234.5)                      # and so does a caller's finite pattern
    assert (pattern[2] == np.float32(-1234.5)).all() and not (pattern[:2] == np.float32(-1234.5)).any()
    check_inside_bound(c.replace(count=5), "3x3 128 -> 128, count above n")


@pytest.mark.parametrize("name", ["heavy_tail", "small_times_large"])
def test_other_families_stay_inside_the_bound(gpu_required, name):
    check_inside_bound(make(name, 2, 14, 14, 64, 128, 3, seed=9), name, variants=(-1,))
    check_inside_bound(make(name, 1, 12, 12, 256, 256, 1, seed=10), name + " 256 rows")


def test_power_of_two_factors_pass_through_bit_for_bit(gpu_required):
    c = make("gaussian", 2, 14, 14, 64, 128, 3, seed=1, bias=False)
    base = c.run_split(-1)
    got = c.replace(x=torch.ldexp(c.x, torch.tensor(-30)), w=torch.ldexp(c.w, torch.tensor(10))).run_split(-1)
    want = np.ldexp(base, -20).astype(np.float32)
    assert float(np.abs(want[want != 0]).min()) >= 2.0 ** -126      # no result left the normal range: the factor is exact on every one
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_zero_input_gives_exactly_relu_of_the_bias(gpu_required, base3x3):
    c, _ = base3x3
    got = c.replace(x=torch.zeros_like(c.x), relu=True).run_split(-1)
    want = np.broadcast_to(np.maximum(c.bias.numpy(), 0)[None, :, None, None], got.shape).astype(np.float32)
    assert (c.bias < 0).any() and (c.bias > 0).any()
    assert same_bits(got, np.ascontiguousarray(want))


def test_one_nan_reaches_exactly_the_outputs_whose_taps_read_it(gpu_required, base3x3):
    c, _ = base3x3
    bad = c.x.clone()
    bad[1, 37, 5, 9] = NAN
    got = c.replace(x=bad).run_split(-1)
    hit = np.zeros(got.shape, bool)
    hit[1, :, 4:7, 8:11] = True
    assert np.isnan(got[hit]).all()
    assert np.isfinite(got[~hit]).all()


def test_two_calls_give_the_same_bits(gpu_required, base3x3):
    c, base = base3x3
    assert same_bits(c.run_split(-1), base)


# ---------------------------------------------------------------------------------------------------------------- the assembled step
def test_assembled_step_in_both_modes(gpu_required):
    """The setting of test_reference_precision_training_step_matches_autograd (256 x 256 tiles, batch 2, sampling 256 / 0.5 / 64 / 0.25, seed 5)
    on ONE fp32 trainer, in fwd modes f32, split, split, f32, then one step with fwd, dgrad and wgrad all split.  In every split step,
    against fp32 autograd on the engine's own samples of that step: the five losses to 1e-4 |ref| + 1e-7 and every weight gradient to
    1e-3 relative L2, the existing test's bars.  The second split step repeats the first one's bits, the f32 step comes back bit for bit,
    and the stage names do not depend on the mode.  The distance between the modes is printed, not asserted: the proposals may differ
    between the modes at NMS near-ties."""
    from oracle import train_oracle as T
    from tests.test_gpu_trainer import _d2_grad, _engine_step, _oracle_losses_on_engine_samples, _two_image_problem, trainable_layers
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision="fp32")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _two_image_problem()
    layers = list(trainable_layers(spec))
    names = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=1.0)

    def step(fwd, dgrad="f32", wgrad="f32"):
        tr.set_fwd_mode(fwd)
        tr.set_dgrad_mode(dgrad)
        tr.set_wgrad_mode(wgrad)
        targets, where = _engine_step(tr, tiles, gt_boxes, gt_classes, polys, seed=5)
        out = {"losses": tr.tensor("losses")[:5].copy()}
        for layer in layers:
            out[f"g:{layer}.w"] = tr.tensor(f"g:{layer}.w").copy()
            try:
                out[f"g:{layer}.b"] = tr.tensor(f"g:{layer}.b").copy()
            except RsError:
                pass                                  # FrozenBN layers have no trainable bias
        return out, targets, where

    def against_autograd(s, targets, where, tag):
        W = {k2: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k2, v in Wn.items()}
        for k2 in T.trainable_keys(W):
            W[k2].requires_grad_(True)
        losses, ref = _oracle_losses_on_engine_samples(tr, spec, W, gt_boxes, polys, targets, where)
        sum(ref[n] for n in names).backward()
        worst = {}
        for layer in layers:
            want = _d2_grad(W, layer, spec)
            worst[layer] = float(np.linalg.norm(s[f"g:{layer}.w"] - want) / max(np.linalg.norm(want), 1e-30))
        top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
        for i, n in enumerate(names):
            r = float(ref[n].detach())
            print(f"{tag}: {n} {float(losses[i]):.8e} against autograd {r:.8e} (|diff| / bar {abs(float(losses[i]) - r) / (1e-4 * abs(r) + 1e-7):.3f})")
        print(f"{tag}: worst weight-gradient rel L2 against autograd:", [(k2.split(".", 2)[-1], f"{v:.2e}") for k2, v in top])
        for i, n in enumerate(names):
            r = float(ref[n].detach())
            assert abs(float(losses[i]) - r) <= 1e-4 * abs(r) + 1e-7, (tag, n, float(losses[i]), r)
        assert max(worst.values()) <= 1e-3, (tag, top)

    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        stages_f32 = [s["name"] for s in tr.stage_times()]
        a, _, _ = step("f32")
        b, targets, where = step("split")
        assert tr.fwd == "split"
        assert [s["name"] for s in tr.stage_times()] == stages_f32
        against_autograd(b, targets, where, "fwd split")       # reads the engine's tensors of THIS step: before the next one runs
        dist = {n: float(np.linalg.norm(b[n].astype(np.float64) - a[n]) / max(np.linalg.norm(a[n]), 1e-30)) for n in a}
        for n in sorted(dist, key=lambda n: -dist[n]):
            print(f"fwd split vs f32 rel L2 {dist[n]:.3e}   {n}")
        assert max(dist.values()) > 0.0, "the split mode ran the fp32 kernel"
        c, _, _ = step("split")
        for n in b:
            assert same_bits(b[n], c[n]), f"second split step: {n}"
        d, _, _ = step("f32")
        for n in a:
            assert same_bits(a[n], d[n]), f"back in mode f32: {n}"
        e, targets, where = step("split", "split", "split")
        assert same_bits(e["losses"], b["losses"])             # the forward does not depend on the backward's modes
        against_autograd(e, targets, where, "fwd + dgrad + wgrad split")
        assert [s["name"] for s in tr.stage_times()] == stages_f32
    finally:
        tr.close()


def test_fp16_trainer_refuses_the_split_mode(gpu_required):
    spec = EngineSpec(num_classes=2, min_size_test=256, max_size_test=426)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=256.0)
    try:
        with pytest.raises(RsError, match="rs_trainer_set_fwd_mode"):
            tr.set_fwd_mode("split")
        assert tr.fwd == "f32"
        tr.set_fwd_mode("f32")
        assert tr.lib.rs_trainer_set_fwd_mode(tr._h, 2) < 0
    finally:
        tr.close()


def test_multi_scale_trainer_carries_the_mode_across_copy_state(gpu_required):
    """The 160 px trainer steps in mode split; the 192 px trainer is then built in mode f32 by hand and takes the state: it arrives in
    mode split with planes of the copied weights -- its forward equals that of a trainer switched on directly, bit for bit."""
    spec = EngineSpec(num_classes=2, min_size_test=192, max_size_test=320, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200, precision="fp32")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(1, 128, 128, 3, seed=31)
    ms = MultiScaleTrainer(spec, Wn, (128, 128, 3), [160, 192], batch=1, loss_scale=1.0, fwd="split")
    other = None
    try:
        ms.set_sampling(64, 0.5, 64, 0.25)
        a = ms.select(160)
        assert a.fwd == "split"
        s = 160 / 128
        gb = [np.array([[20.0, 30.0, 90.0, 100.0]], np.float32) * s]
        polys = [[[np.array([20.0, 30, 90, 30, 90, 100, 20, 100]) * s]]]
        l0 = a.train_step(tiles, gb, [np.array([1])], polys, seed=3)
        a.apply_sgd(1e-3, 0.9, 1e-4)
        assert all(np.isfinite(v) for v in l0.values())
        b = ms.select(192)                                   # built with fwd="split", then copy_state: re-split behind the fold
        assert b is not a and b.fwd == "split"
        other = Trainer(spec.replace(min_size_test=192), Wn, (128, 128, 3), batch=1, loss_scale=1.0)      # mode f32
        other.set_sampling(64, 0.5, 64, 0.25)
        assert other.fwd == "f32"
        other.copy_state_from(a)
        assert other.fwd == "split"
        s2 = 192 / 128
        args = (tiles, [gb[0] / s * s2], [np.array([1])], [[[polys[0][0][0] / s * s2]]])
        l1, l2 = b.train_step(*args, seed=4), other.train_step(*args, seed=4)
        assert all(np.isfinite(v) for v in l1.values())
        assert l1 == l2, (l1, l2)
        assert same_bits(b.tensor("losses")[:5].copy(), other.tensor("losses")[:5].copy())
        other.set_fwd_mode("f32")
        l3 = other.train_step(*args, seed=4)
        assert l3 != l2, "the carried mode ran the fp32 kernel"
    finally:
        if other is not None:
            other.close()
        ms.close()


def test_train_model_cli_runs_in_split_mode_and_refuses_it_on_the_fp16_trainer(gpu_required, tmp_path, caplog):
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    cwd = os.getcwd()
    wd = _tiny_training_workdir(tmp_path)
    try:
        with pytest.raises(SystemExit, match="--fwd split"):
            train_model.main([str(tmp_path / "config.yaml"), "--synthetic-weights", "--max-iter", "2", "--precision", "fp16", "--fwd", "split",
                              "--tagged-samples", "0"])
        os.chdir(cwd)
        with caplog.at_level(logging.INFO, logger="train_model"):
            assert train_model.main([str(tmp_path / "config.yaml"), "--fwd", "split", "--max-iter", "2", "--synthetic-weights", "--log-period", "1",
                                     "--tagged-samples", "0"]) == 0
    finally:
        os.chdir(cwd)
    assert any("fwd: split" in r.getMessage() for r in caplog.records)
    lines = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
    assert [l["iteration"] for l in lines] == [0, 1]
    names = ("total_loss", "loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
    assert all(np.isfinite(l[k]) for l in lines for k in names), lines
