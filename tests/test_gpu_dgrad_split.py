"""Input gradients of the fp32 trainer on split operands (csrc/conv_igemm.hip TRAIN && SPLIT, rs_op_conv2d_dgrad_split, rs_op_split_rows,
rs_trainer_set_dgrad_mode, ``Trainer(dgrad="split")``, ``train_model.py --dgrad split``) on the GPU.

The operator is held, per element, to the derived bound of tests/dgrad_split_ref.py plus the accumulation-order error of the fp32
matrix-core kernel, measured inside the test from rs_op_conv2d(use_glds = -1) on the same dy and w_t as a plain stride-1 convolution:

    |gemm - ref64| <= 2^-20 S + 2^-36 T max|dy| rowmax|w| + E_f32          (+ 6 * 2^-24 (|gemm| + sum |addend|) with addends)

Every case runs every tile the dispatch can choose for its row count, by number."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd.engine import RsError, Trainer, _check, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import split_planes, synthetic_weights
from tests.util import synthetic_tiles
from tests import dgrad_split_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def tiles_for(cin):
    """The tile numbers conv_dgrad_split_variant can return for `cin` output rows (-1, the rule itself, runs too)."""
    return (-1, 7, 14, 4) if cin % 256 == 0 else ((-1, 7) if cin % 128 == 0 else (-1, 2))


def _halo(t_nhwc, pad, fill=0.0):
    n, h, w, c = t_nhwc.shape
    out = torch.full((n, h + 2 * pad, w + 2 * pad, c), fill, dtype=torch.float32)
    out[:, pad:pad + h, pad:pad + w] = t_nhwc
    return out


class Case:
    """dy (n, cout, ho, wo), w_t (cin, k, k, cout) -- already transposed and tap-flipped, i.e. the weight of the plain convolution the
    input gradient is -- and optional addends in dx's (n, cin, hi, wi) / the finer map's shape; everything fp32 torch."""

    def __init__(self, dy, w_t, k, stride, pad, hi, wi, res=None, res32=None, mask=None, down=None, halo=1, count=None):
        self.dy, self.w_t, self.k, self.stride, self.pad, self.hi, self.wi = dy, w_t, k, stride, pad, hi, wi
        self.res, self.res32, self.mask, self.down, self.halo, self.count = res, res32, mask, down, halo, count
        self.n, self.cout, self.ho, self.wo = dy.shape
        self.cin = w_t.shape[0]
        self.kpad = k * k * self.cout

    def replace(self, **kw):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    def gemm64(self, absolute=False):
        """(n, cin, hi, wi) float64: the exact product (or S, the same sum over magnitudes); unvisited pixels of a strided case are 0."""
        dy, w = self.dy.double(), self.w_t.double()
        if absolute:
            dy, w = dy.abs(), w.abs()
        y = F.conv2d(dy, w.permute(0, 3, 1, 2), padding=self.k - 1 - self.pad)
        if self.stride == 1:
            return y.numpy()
        out = torch.zeros(self.n, self.cin, self.hi, self.wi, dtype=torch.float64)
        out[:, :, ::self.stride, ::self.stride][:, :, :self.ho, :self.wo] = y
        return out.numpy()

    def addends(self):
        out = [a for a in (self.res, self.res32) if a is not None]
        if self.down is not None:
            d = self.down
            out[1:1] = [d[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
        return out

    def run_split(self, variant=-1, fill=NAN):
        """dx (n, cin, hi, wi) fp32 from rs_op_conv2d_dgrad_split; dx starts as `fill` everywhere, halo included."""
        lib = load_library()
        h = self.halo
        up = lambda t, p=h: None if t is None else _halo(t.permute(0, 2, 3, 1).float().contiguous(), p).to(DEV)
        dyd, res, res32, mask, down = up(self.dy), up(self.res), up(self.res32), up(self.mask), up(self.down)
        wd = self.w_t.reshape(self.cin, self.kpad).contiguous().to(DEV)
        dxd = torch.full((self.n, self.hi + 2 * h, self.wi + 2 * h, self.cin), fill, dtype=torch.float32, device=DEV)
        cnt = torch.tensor([self.count], dtype=torch.int32, device=DEV) if self.count is not None else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        torch.cuda.synchronize()
        rc = lib.rs_op_conv2d_dgrad_split(ptr(dyd), ptr(wd), ptr(dxd), ptr(res), ptr(res32), ptr(mask), ptr(down), self.n, self.hi, self.wi, self.cin,
                                          self.ho, self.wo, self.cout, self.k, self.k, self.stride, self.pad, self.kpad, h, variant, ptr(cnt), None)
        _check(lib, rc, "rs_op_conv2d_dgrad_split")
        torch.cuda.synchronize()
        full = dxd.cpu()
        ring = torch.ones(full.shape[1:3], dtype=torch.bool)
        ring[h:h + self.hi, h:h + self.wi] = False
        self.last_halo_untouched = bool(torch.isnan(full[:, ring]).all()) if fill != fill else True
        return full[:, h:h + self.hi, h:h + self.wi].permute(0, 3, 1, 2).contiguous().numpy()

    def e_f32(self, ref):
        """Largest error of the fp32 matrix-core kernel on the same product (a plain stride-1 convolution of dy with w_t) against float64."""
        lib = load_library()
        h, pt = self.halo, self.k - 1 - self.pad
        dyd = _halo(self.dy.permute(0, 2, 3, 1).float().contiguous(), h).to(DEV)
        wd = self.w_t.reshape(self.cin, self.kpad).contiguous().to(DEV)
        oh, ow = self.ho + 2 * pt - self.k + 1, self.wo + 2 * pt - self.k + 1
        out = torch.zeros((self.n, oh + 2 * h, ow + 2 * h, self.cin), dtype=torch.float32, device=DEV)
        bias = torch.zeros(self.cin + 64, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        rc = lib.rs_op_conv2d(C.c_void_p(dyd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(bias.data_ptr()), C.c_void_p(out.data_ptr()), None, None,
                              self.n, self.ho, self.wo, self.cout, h, self.k, self.k, 1, pt, self.cin, self.kpad, h, 0, 1, 0, -1, -1, None)
        _check(lib, rc, "rs_op_conv2d (fp32)")
        torch.cuda.synchronize()
        got = out.cpu()[:, h:h + oh, h:h + ow].permute(0, 3, 1, 2).double().numpy()
        want = ref if self.stride == 1 else ref[:, :, ::self.stride, ::self.stride][:, :, :self.ho, :self.wo]
        return float(np.abs(got - want).max())


def make(name, n, ho, wo, cout, cin, k, stride=1, pad=None, halo=1, seed=0, real_cout=None):
    pad = k // 2 if pad is None else pad
    rng = np.random.default_rng(1000 + seed)
    dy, w = R.family(name, rng, (n, cout, ho, wo), (cin, k, k, cout))
    if real_cout is not None:                    # a narrow head: the K side is padded with zero channels (and zero weight columns)
        dy[:, real_cout:] = 0
        w[..., real_cout:] = 0
    hi, wi = (ho, wo) if stride == 1 else (ho * stride, wo * stride)
    return Case(torch.as_tensor(dy), torch.as_tensor(w), k, stride, pad, hi, wi, halo=halo)


def check_inside_bound(c, tag, variants=None):
    """Every tile of the case inside the per-element bound, on a NaN-filled dx; returns the results by tile number."""
    ref, S = c.gemm64(), c.gemm64(absolute=True)
    e32 = c.e_f32(ref)
    fin = c.dy[torch.isfinite(c.dy)]
    lim = R.bound(S.transpose(0, 2, 3, 1).reshape(-1, c.cin), c.kpad, float(fin.abs().max()), c.w_t.reshape(c.cin, -1).abs().max(dim=1).values.numpy())
    lim = lim.reshape(c.n, c.hi, c.wi, c.cin).transpose(0, 3, 1, 2) + e32
    adds = c.addends()
    want = ref.copy()
    if adds:
        lim = lim + R.epilogue_allowance(ref, sum(a.double().abs().numpy() for a in adds))
        want = want + sum(a.double().numpy() for a in adds)
    visited = np.zeros((c.hi, c.wi), bool)
    visited[::c.stride, ::c.stride][:c.ho, :c.wo] = True
    live = np.broadcast_to(visited[None, None], want.shape).copy()
    if c.count is not None:
        live[c.count:] = False
    keep = live if c.mask is None else live & (c.mask.numpy() > 0)
    out = {}
    for v in variants or tiles_for(c.cin):
        got = c.run_split(v)
        assert c.last_halo_untouched, f"{tag} tile {v}: the halo of dx was written"
        assert np.isnan(got[~live]).all(), f"{tag} tile {v}: an element outside the launch was written"
        assert np.isfinite(got[live]).all(), f"{tag} tile {v}: {int((~np.isfinite(got[live])).sum())} elements not written or not finite"
        if c.mask is not None:
            zero = live & ~keep
            assert zero.any() and np.array_equal(got[zero].view(np.uint32), np.zeros(int(zero.sum()), np.uint32)), f"{tag} tile {v}: masked elements are not +0"
        err = np.abs(got.astype(np.float64) - want)[keep]
        used = float((err / lim[keep]).max())
        print(f"{tag} tile {v}: max err {err.max():.3e} (fp32 kernel {e32:.3e}), largest err / bound {used:.3f}")
        assert used <= 1.0, (tag, v, used)
        out[v] = got
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_split_rows_equals_weights_split_planes_bit_for_bit(gpu_required):
    lib = load_library()
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((96, 576)) * np.exp2(rng.uniform(-20, 20, (96, 1)))).astype(np.float32)
    w[5] = 0
    w[17] = 1e-30
    wd = torch.as_tensor(w).to(DEV)
    planes = torch.full((2 * 96, 576), NAN, dtype=torch.float16, device=DEV)
    inv = torch.full((96,), NAN, dtype=torch.float32, device=DEV)
    _check(lib, lib.rs_op_split_rows(C.c_void_p(wd.data_ptr()), 96, 576, C.c_void_p(planes.data_ptr()), C.c_void_p(inv.data_ptr()), None), "rs_op_split_rows")
    torch.cuda.synchronize()
    want_planes, want_inv = split_planes(w)
    assert np.array_equal(planes.cpu().numpy().view(np.uint16), want_planes.view(np.uint16))
    assert np.array_equal(inv.cpu().numpy().view(np.uint32), want_inv.view(np.uint32))


@pytest.fixture(scope="module")
def base3x3():
    c = make("gaussian", 2, 14, 14, 128, 64, 3, seed=1)
    return c, c.run_split(-1)


def test_3x3_and_its_every_tile(gpu_required, base3x3):
    c, base = base3x3
    got = check_inside_bound(c, "3x3 128 -> 64")
    for v, g in got.items():
        assert same_bits(g, base), f"tile {v} and the rule's tile differ"


def test_1x1(gpu_required):
    check_inside_bound(make("gaussian", 2, 14, 14, 256, 64, 1, seed=2), "1x1 256 -> 64")


def test_1x1_stride_2_leaves_unvisited_pixels_alone(gpu_required):
    c = make("gaussian", 1, 7, 7, 128, 256, 1, stride=2, seed=3)
    got = check_inside_bound(c, "1x1 s2 128 -> 256")              # NaN fill: every unvisited pixel is still NaN
    pattern = c.run_split(-1, fill=-1234.5)                       # and a caller's finite pattern survives bit for bit
    assert (pattern[:, :, 1::2, :] == np.float32(-1234.5)).all() and (pattern[:, :, :, 1::2] == np.float32(-1234.5)).all()
    assert same_bits(pattern[:, :, ::2, ::2], got[-1][:, :, ::2, ::2])
    assert all(same_bits(g[:, :, ::2, ::2], got[-1][:, :, ::2, ::2]) for g in got.values())      # an output's bits do not depend on its tile


def test_3x3_with_all_addends_and_the_mask(gpu_required, base3x3):
    c, _ = base3x3
    g = torch.Generator().manual_seed(11)
    shape = (c.n, c.cin, c.hi, c.wi)
    check_inside_bound(c.replace(res=torch.randn(shape, generator=g), res32=torch.randn(shape, generator=g) * 0.3, mask=torch.randn(shape, generator=g)),
                       "3x3 + res + res32 + mask")


def test_down_adds_the_2x2_sums_of_the_finer_map(gpu_required):
    c = make("gaussian", 2, 8, 8, 64, 128, 1, seed=5)
    g = torch.Generator().manual_seed(12)
    check_inside_bound(c.replace(down=torch.randn((2, 128, 16, 16), generator=g)), "1x1 + down")


def test_fc_as_an_m_by_1_image(gpu_required):
    check_inside_bound(make("gaussian", 1, 70, 1, 1024, 256, 1, halo=0, seed=6), "fc 70 x 1024 -> 256")


def test_16_row_head_padded_to_64_on_the_k_side(gpu_required):
    check_inside_bound(make("gaussian", 2, 14, 14, 64, 256, 1, seed=7, real_cout=16), "head 16 (64) -> 256")


def test_count_bounded_launch_writes_its_images_only(gpu_required):
    c = make("gaussian", 3, 9, 11, 128, 128, 3, seed=8)
    check_inside_bound(c.replace(count=2), "3x3 128 -> 128, 2 of 3 images")
    check_inside_bound(c.replace(count=5), "3x3 128 -> 128, count above n")


@pytest.mark.parametrize("name", ["heavy_tail", "small_times_large"])
def test_other_families_stay_inside_the_bound(gpu_required, name):
    check_inside_bound(make(name, 2, 14, 14, 128, 64, 3, seed=9), name, variants=(-1,))
    check_inside_bound(make(name, 1, 12, 12, 64, 256, 1, seed=10), name + " 256 rows")


def test_power_of_two_factors_pass_through_bit_for_bit(gpu_required, base3x3):
    c, base = base3x3
    got = c.replace(dy=torch.ldexp(c.dy, torch.tensor(-30)), w_t=torch.ldexp(c.w_t, torch.tensor(10))).run_split(-1)
    want = np.ldexp(base, -20).astype(np.float32)
    assert float(np.abs(want[want != 0]).min()) >= 2.0 ** -126      # no result left the normal range: the factor is exact on every one
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def test_zero_gradient_gives_exact_zeros(gpu_required, base3x3):
    c, _ = base3x3
    got = c.replace(dy=torch.zeros_like(c.dy)).run_split(-1)
    assert same_bits(got, np.zeros_like(got))


def test_one_nan_reaches_exactly_the_outputs_whose_taps_read_it(gpu_required, base3x3):
    c, _ = base3x3
    bad = c.dy.clone()
    bad[1, 77, 5, 9] = NAN
    got = c.replace(dy=bad).run_split(-1)
    hit = np.zeros(got.shape, bool)
    hit[1, :, 4:7, 8:11] = True
    assert np.isnan(got[hit]).all()
    assert np.isfinite(got[~hit]).all()


def test_two_calls_give_the_same_bits(gpu_required, base3x3):
    c, base = base3x3
    assert same_bits(c.run_split(-1), base)


# ---------------------------------------------------------------------------------------------------------------- the assembled step
# Relative L2 distance between a gradient tensor of dgrad mode split and of mode f32: 4x the worst value measured on an MI355X over the
# 80 weight- and bias-gradient tensors of this step (profiles/dgrad_split/README.md, assembled_step_mode_distance.txt): 3.930e-6
# (res3.0.conv1.w, the end of the longest chain of input gradients) down to 6.6e-8 (fc2), and exactly 0 for the three heads whose dY
# comes straight from a loss.  The weight-gradient mode's 1.6e-7 was one product's error; here every stage adds its own along the chain.
MEASURED_WORST_MODE_DISTANCE = 3.930e-6


def test_assembled_step_in_both_modes(gpu_required):
    """The setting of test_reference_precision_training_step_matches_autograd (256 x 256 tiles, batch 2, sampling 256 / 0.5 / 64 / 0.25, seed 5)
    on ONE fp32 trainer, in dgrad modes f32, split, split, f32, then one step with wgrad and dgrad both split.  The forward is untouched:
    the five losses are bit-identical in all of them.  In split mode every weight gradient is within 1e-3 relative L2 of autograd (the
    existing bar), with the weight gradients split as well too; a second split step repeats the first one's bits and the f32 step comes
    back bit for bit.  The distance between the modes is printed per tensor and bounded by 4x the worst value measured, 1.572e-5.
    Against autograd the worst tensor is 4.62e-4 (res5.2.conv1) in mode split and with both products split alike."""
    from oracle import train_oracle as T
    from tests.test_gpu_trainer import _d2_grad, _engine_step, _oracle_losses_on_engine_samples, _two_image_problem, trainable_layers
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision="fp32")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _two_image_problem()
    layers = list(trainable_layers(spec))
    tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=1.0)

    def step(dgrad, wgrad="f32"):
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

    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        a, _, _ = step("f32")
        b, targets, where = step("split")
        assert tr.dgrad == "split"
        assert same_bits(a["losses"], b["losses"]), (a["losses"], b["losses"])
        W = {k2: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k2, v in Wn.items()}
        for k2 in T.trainable_keys(W):
            W[k2].requires_grad_(True)
        _, ref = _oracle_losses_on_engine_samples(tr, spec, W, gt_boxes, polys, targets, where)
        sum(ref[n] for n in ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")).backward()
        want = {layer: _d2_grad(W, layer, spec) for layer in layers}
        against_autograd = lambda s: {layer: float(np.linalg.norm(s[f"g:{layer}.w"] - want[layer]) / max(np.linalg.norm(want[layer]), 1e-30)) for layer in layers}
        worst = against_autograd(b)
        dist = {n: float(np.linalg.norm(b[n].astype(np.float64) - a[n]) / max(np.linalg.norm(a[n]), 1e-30)) for n in a if n != "losses"}
        for n in sorted(dist, key=lambda n: -dist[n]):
            layer = n[2:-2]
            print(f"dgrad split vs f32 rel L2 {dist[n]:.3e}   split vs autograd {worst[layer] if n.endswith('.w') else float('nan'):.3e}   {n}")
        assert max(worst.values()) <= 1e-3, sorted(worst.items(), key=lambda kv: -kv[1])[:6]
        assert max(dist.values()) > 0.0, "the split mode ran the fp32 kernel"
        assert max(dist.values()) <= 4 * MEASURED_WORST_MODE_DISTANCE, sorted(dist.items(), key=lambda kv: -kv[1])[:6]
        c, _, _ = step("split")
        for n in b:
            assert same_bits(b[n], c[n]), f"second split step: {n}"
        d, _, _ = step("f32")
        for n in a:
            assert same_bits(a[n], d[n]), f"back in mode f32: {n}"
        e, _, _ = step("split", "split")
        assert same_bits(a["losses"], e["losses"])
        both = against_autograd(e)
        print(f"wgrad + dgrad split: worst against autograd {max(both.values()):.3e} ({max(both, key=both.get)})")
        assert max(both.values()) <= 1e-3, sorted(both.items(), key=lambda kv: -kv[1])[:6]
    finally:
        tr.close()


def test_fp16_trainer_refuses_the_split_mode(gpu_required):
    spec = EngineSpec(num_classes=2, min_size_test=256, max_size_test=426)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=256.0)
    try:
        with pytest.raises(RsError, match="rs_trainer_set_dgrad_mode"):
            tr.set_dgrad_mode("split")
        assert tr.dgrad == "f32"
        tr.set_dgrad_mode("f32")
        assert tr.lib.rs_trainer_set_dgrad_mode(tr._h, 2) < 0
    finally:
        tr.close()


def test_train_model_cli_refuses_the_switch_on_the_fp16_trainer(gpu_required, tmp_path):
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    cwd = os.getcwd()
    _tiny_training_workdir(tmp_path)
    try:
        with pytest.raises(SystemExit, match="--dgrad split"):
            train_model.main([str(tmp_path / "config.yaml"), "--synthetic-weights", "--max-iter", "2", "--precision", "fp16", "--dgrad", "split",
                              "--tagged-samples", "0"])
    finally:
        os.chdir(cwd)
