"""The segmented optimiser step on the GPU: rs_op_sgd_segments (grad_norm_partial_kernel, grad_norm_finish_kernel, sgd_segments_kernel)
on synthetic segment tables against the float64 rule of tests/solver_ref.py, and the assembled trainer with a solver set -- norms,
coefficients and master weights after rs_trainer_apply_sgd, the default path bit for bit, the tensor table, the stem's padding columns,
and one train_model run with ``--solver extended``.

Bounds (solver_ref.bounds): a norm within 2^-22 relative of float64 numpy (float64 accumulation, one fp32 rounding,
sqrtf), the inf norm exact, a coefficient within 2^-21, and -- given the kernel's own coefficients read back -- every weight within
2^-21 (|w| + lr (1 + mu) (mu |buf| + |g~| + wd |w|)) of the float64 rule, the momentum buffer within 2^-21 (mu |buf| + |g~| + wd |w|)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import RsError, SolverOptions, Trainer, _check, load_library
from proj_roadsurf_amd.weights import synthetic_weights
from tests import solver_ref as R
from tests.test_gpu_train_classes import _problem, _spec
from tests.util import synthetic_tiles

pytestmark = pytest.mark.gpu

INV = 1.0 / 512.0
LR, MU, WD = 0.01, 0.9, 1e-4
COUNTS = [1, 3, 63, 64, 65, 255, 256, 257, R.CHUNK, R.CHUNK + 1, 3 * R.CHUNK + 5]
GAPS = [0, 4, 12, R.CHUNK + 20]          # beyond the next multiple of 4: none is a multiple of the chunk; one is longer than a chunk
ZERO = 4                                  # the all-zero segment


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _op(lib, w, buf, grad, segs, opts, lr=LR, mu=MU, wd=WD, inv=INV, skip=None, check=True):
    """rs_op_sgd_segments on device copies -> (rc, w, buf, norms, coef) on the host."""
    dw, db, dg = (torch.from_numpy(np.array(a, np.float32)).to("cuda:0") for a in (w, buf, grad))
    dn, dc = (torch.full((max(len(segs), 1),), -1.0, dtype=torch.float32, device="cuda:0") for _ in range(2))
    ds = None if skip is None else torch.tensor([skip], dtype=torch.int32, device="cuda:0")
    off = np.array([s[0] for s in segs], np.int64)
    cnt = np.array([s[1] for s in segs], np.int64)
    fl = np.array([s[2] for s in segs], np.int32)
    st = opts.to_struct()
    torch.cuda.synchronize()
    rc = lib.rs_op_sgd_segments(_vp(dw), _vp(db), _vp(dg), len(w), off.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                fl.ctypes.data_as(C.c_void_p), len(segs), lr, mu, wd, inv, C.byref(st), _vp(ds), _vp(dn), _vp(dc), None)
    if check:
        _check(lib, rc, "rs_op_sgd_segments")
    torch.cuda.synchronize()
    return rc, dw.cpu().numpy(), db.cpu().numpy(), dn.cpu().numpy()[:len(segs)], dc.cpu().numpy()[:len(segs)]


@pytest.fixture(scope="module")
def lib(gpu_required):
    return load_library()


@pytest.fixture(scope="module")
def case():
    """One table, one set of buffers, shared and left unchanged; gradients for the L2 and for the inf norm."""
    rng = np.random.default_rng(21)
    segs, n = R.table(COUNTS, GAPS)
    assert all(o % 4 == 0 for o, _, _ in segs) and any((o + c) % 4 for o, c, _ in segs)
    w, buf = rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32)
    grad = {nt: R.gradients(rng, segs, n, INV, 1.0, ZERO, norm_type=nt) for nt in (2.0, math.inf)}
    for a in (w, buf, grad[2.0], grad[math.inf]):
        a.setflags(write=False)
    return dict(segs=segs, n=n, w=w, buf=buf, grad=grad)


# ------------------------------------------------------------------ the operator

def test_defaults_equal_the_plain_step_bit_for_bit_gaps_included(lib, case):
    """(a) c = 1 everywhere, no Nesterov, factor 1: rs_op_sgd_momentum's bits over every element of the buffer."""
    w, buf, grad = case["w"], case["buf"], case["grad"][2.0]
    dw, db, dg = (torch.from_numpy(a.copy()).to("cuda:0") for a in (w, buf, grad))
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_sgd_momentum(_vp(dw), _vp(db), _vp(dg), len(w), LR, MU, WD, INV, 0, None), "rs_op_sgd_momentum")
    torch.cuda.synchronize()
    _, w1, b1, norms, coef = _op(lib, w, buf, grad, case["segs"], SolverOptions())
    assert not np.array_equal(w1, w) and np.array_equal(_bits(w1), _bits(dw.cpu().numpy())) and np.array_equal(_bits(b1), _bits(db.cpu().numpy()))
    assert (norms == -1).all() and (coef == -1).all()                       # no norm pass without a norm to clip by
    # the fp32 restatement states the same bits
    want_w, want_b = R.rule(w, buf, grad, INV, LR, WD, MU, False)
    assert np.array_equal(_bits(w1), _bits(want_w)) and np.array_equal(_bits(b1), _bits(want_b))


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("mode,norm_type", [("norm", 2.0), ("norm", math.inf), ("full_model", 2.0), ("full_model", math.inf)],
                         ids=["norm-2", "norm-inf", "full_model-2", "full_model-inf"])
def test_norms_coefficients_and_update_against_float64(lib, case, mode, norm_type, nesterov):
    """(b)"""
    segs, w, buf, grad = case["segs"], case["w"], case["buf"], case["grad"][norm_type]
    opts = SolverOptions(nesterov=nesterov, bias_lr_factor=2.0, weight_decay_bias=0.0, clip_type=mode, clip_value=1.0, norm_type=norm_type)
    _, w1, b1, norms, coef = _op(lib, w, buf, grad, segs, opts)
    n64 = R.norms64(grad, INV, segs, norm_type)
    rel = np.abs(norms - n64) / np.maximum(n64, 1e-300)
    print(f"{mode} {norm_type:g}: worst norm error {rel.max() / R.U22:.3f} x 2^-22")
    assert norms[ZERO] == 0 and (rel <= R.U22).all()
    if np.isinf(norm_type):
        assert np.array_equal(norms, n64.astype(np.float32))                # the largest magnitude is an fp32 value: exact
    if mode == "norm":
        c64 = R.coef64(n64, 1.0)
        assert coef[ZERO] == 1 and (coef == 1).sum() >= 3 and (coef < 1).sum() >= 3      # below, above, and 1 / 1e-6 clamped
    else:
        c64 = np.full(len(segs), R.coef64(R.total64(n64, norm_type), 1.0))
        assert (coef == coef[0]).all() and coef[0] < 1
    crel = np.abs(coef - c64) / c64
    print(f"   worst coefficient error {crel.max() / R.U21:.3f} x 2^-21")
    assert (crel <= R.U21).all()
    w64, b64, tw, tb = R.step64(w, buf, grad, segs, INV, LR, MU, WD, nesterov, 2.0, 0.0, mode, 1.0, coef=coef)
    ew, eb = np.abs(w1 - w64), np.abs(b1 - b64)
    print(f"   worst weight error / bound {(ew / np.maximum(tw, 1e-300)).max():.3f}, momentum {(eb / np.maximum(tb, 1e-300)).max():.3f}")
    assert (ew <= tw).all() and (eb <= tb).all()
    # and the rule itself, in fp32 with the kernel's coefficients, bit for bit (no contraction anywhere)
    want_w, want_b = R.rule(w, buf, grad, INV, LR, WD, MU, nesterov)
    for i, (off, cnt, flag) in enumerate(segs):
        s = slice(off, off + cnt)
        lr_s, wd_s = (np.float32(LR) * np.float32(2.0), 0.0) if flag else (LR, WD)
        want_w[s], want_b[s] = R.rule(w[s], buf[s], grad[s], INV, lr_s, wd_s, MU, nesterov, coef=coef[i])
    assert np.array_equal(_bits(w1), _bits(want_w)) and np.array_equal(_bits(b1), _bits(want_b))


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
def test_value_clipping_at_the_threshold_and_just_beyond(lib, case, nesterov):
    """(c) gradients exactly at +-v stay, the next fp32 value beyond is clamped, the one inside is not; every segment, gaps untouched by the
    clamp."""
    segs, w, buf = case["segs"], case["w"], case["buf"]
    v = np.float32(0.375)
    grad = case["grad"][2.0].copy()
    edge = np.array([v, -v, np.nextafter(v, np.float32(1)), -np.nextafter(v, np.float32(1)), np.nextafter(v, np.float32(0)),
                     -np.nextafter(v, np.float32(0)), 4 * v, -4 * v, 0.0], np.float32) / np.float32(INV)
    for off, cnt, _ in segs:
        k = min(cnt, len(edge))
        grad[off + cnt - k:off + cnt] = edge[:k]                            # at the end: the scalar tail of the last chunk too
    gap = segs[1][0] - 1                                                     # a value in no segment, far above v
    grad[gap] = np.float32(100.0) / np.float32(INV)
    opts = SolverOptions(nesterov=nesterov, bias_lr_factor=2.0, weight_decay_bias=0.0, clip_type="value", clip_value=float(v))
    _, w1, b1, norms, _ = _op(lib, w, buf, grad, segs, opts)
    w64, b64, tw, tb = R.step64(w, buf, grad, segs, INV, LR, MU, WD, nesterov, 2.0, 0.0, "value", float(v))
    assert (np.abs(w1 - w64) <= tw).all() and (np.abs(b1 - b64) <= tb).all() and (norms == -1).all()
    want_w, want_b = R.rule(w, buf, grad, INV, LR, WD, MU, nesterov)
    for off, cnt, flag in segs:
        s = slice(off, off + cnt)
        lr_s, wd_s = (np.float32(LR) * np.float32(2.0), 0.0) if flag else (LR, WD)
        want_w[s], want_b[s] = R.rule(w[s], buf[s], grad[s], INV, lr_s, wd_s, MU, nesterov, clamp=v)
    assert np.array_equal(_bits(w1), _bits(want_w)) and np.array_equal(_bits(b1), _bits(want_b))
    # spelled out on the last segment (a weight: wd * w enters): with no Nesterov buf = mu * buf + (clamp(g) + wd * w)
    off, cnt, flag = segs[-1]
    assert flag == 0
    i = np.arange(off + cnt - len(edge), off + cnt)
    clamped = np.clip(edge * np.float32(INV), -v, v)
    assert np.array_equal(clamped[:4], [v, -v, v, -v]) and abs(clamped[4]) < v and np.array_equal(clamped[6:8], [v, -v])
    assert np.array_equal(_bits(b1[i]), _bits(np.float32(MU) * buf[i] + (clamped + np.float32(WD) * w[i])))
    assert abs(b1[gap] - (MU * buf[gap] + 100.0 + WD * w[gap])) < 1e-3                  # the gap is not clipped


def test_skip_leaves_weights_and_momentum_bit_unchanged(lib, case):
    """(d)"""
    for mode in ("none", "value", "norm", "full_model"):
        _, w1, b1, norms, _ = _op(lib, case["w"], case["buf"], case["grad"][2.0], case["segs"], SolverOptions(nesterov=True, clip_type=mode, bias_lr_factor=2.0), skip=1)
        assert np.array_equal(_bits(w1), _bits(case["w"])) and np.array_equal(_bits(b1), _bits(case["buf"])), mode
        assert (norms >= 0).all() == (mode in ("norm", "full_model"))      # the norms are still measured
    _, w1, _, _, _ = _op(lib, case["w"], case["buf"], case["grad"][2.0], case["segs"], SolverOptions(clip_type="norm"), skip=0)
    assert not np.array_equal(w1, case["w"])


@pytest.mark.parametrize("mode,norm_type", [("norm", 2.0), ("full_model", 2.0), ("norm", math.inf)], ids=["norm-2", "full_model-2", "norm-inf"])
def test_two_runs_give_the_same_bits(lib, case, mode, norm_type):
    """(e)"""
    opts = SolverOptions(nesterov=True, bias_lr_factor=2.0, clip_type=mode, clip_value=1.0, norm_type=norm_type)
    a = _op(lib, case["w"], case["buf"], case["grad"][norm_type], case["segs"], opts)
    b = _op(lib, case["w"], case["buf"], case["grad"][norm_type], case["segs"], opts)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(_bits(x), _bits(y))


def test_bad_table_returns_rs_err_arg(lib, case):
    """(f)"""
    w, buf, grad = (np.ones(64, np.float32) for _ in range(3))
    for segs in ([(2, 8, 0)], [(0, 0, 0)], [(0, 65, 0)], [(60, 8, 0)], [(8, 8, 0), (12, 4, 0)], [(16, 4, 0), (0, 4, 0)], [(0, 4, 2)], []):
        rc, w1, b1, _, _ = _op(lib, w, buf, grad, segs, SolverOptions(clip_type="norm"), check=False)
        assert rc == -1 and b"rs_op_sgd_segments" in lib.rs_last_error(), (segs, lib.rs_last_error())
        assert np.array_equal(w1, w) and np.array_equal(b1, buf)
    rc, _, _, _, _ = _op(lib, w, buf, grad, [(0, 8, 0)], SolverOptions(nesterov=True), mu=0.0, check=False)
    assert rc == -1 and b"momentum" in lib.rs_last_error()


# ------------------------------------------------------------------ the assembled trainer

def _segment_norms(tr, segs, scale):
    """float64 L2 norm of every trainable tensor's unscaled gradient, from the "g:" tensors."""
    return np.array([np.sqrt(np.sum((tr.tensor("g:" + name).astype(np.float64) / scale) ** 2)) for name, _, _, _ in segs])


@pytest.fixture(scope="module", params=["fp32", "fp16"])
def assembled(request, gpu_required):
    """One trainer at 256 x 256, batch 2 (fp16: loss scale 256).  Step 1 runs with no solver, which also yields the momentum buffer (from
    zero, buf = g * inv + wd * w: the fp32 restatement gives its bits, checked on the weights).  Step 2 runs per-tensor norm clipping at
    the median norm with Nesterov and BIAS_LR_FACTOR 2; step 3 full_model."""
    precision = request.param
    scale = 1.0 if precision == "fp32" else 256.0
    spec = _spec(3, precision)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem(3)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=scale)
    out = dict(precision=precision, scale=scale)
    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        out["names_unset"] = tr.tensor_names()
        segs = out["segs"] = tr.segments()
        tab = [(o, c, int(b)) for _, o, c, b in segs]
        inv = np.float32(1.0) / np.float32(scale)
        # step 1: no solver
        tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5)
        m0, g1 = tr.flat("master").copy(), tr.flat("grad").copy()
        tr.apply_sgd(LR, MU, WD)
        out["overflow1"] = tr.overflowed()
        m1 = tr.flat("master").copy()
        want_m1, buf1 = R.rule(m0, np.zeros_like(m0), g1, inv, LR, WD, MU, False)
        out["plain_step_is_the_restatement"] = np.array_equal(_bits(m1), _bits(want_m1))
        # step 2: norm clipping at the median, Nesterov, bias factor 2
        tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=6)
        g2 = tr.flat("grad").copy()
        n64 = _segment_norms(tr, segs, scale)
        assert np.allclose(n64, R.norms64(g2, inv, tab), rtol=1e-12)        # the "g:" tensors are the segments of the flat buffer
        max_norm = float(np.float32(np.median(n64)))
        tr.set_solver(SolverOptions(nesterov=True, bias_lr_factor=2.0, clip_type="norm", clip_value=max_norm))
        out["names_set"] = tr.tensor_names()
        tr.apply_sgd(LR, MU, WD)
        out["overflow2"] = tr.overflowed()
        out.update(n64=n64, max_norm=max_norm, norms=tr.tensor("grad_norms").copy(), coef=tr.tensor("clip_coef").copy(), by_name=tr.grad_norms())
        m2 = tr.flat("master").copy()
        out["m2"] = m2
        out["want2"] = R.step64(m1, buf1, g2, tab, inv, LR, MU, WD, True, 2.0, None, "norm", max_norm, coef=out["coef"])
        out["m_tensors"] = {name: tr.tensor("m:" + name).copy() for name, _, _, _ in segs[:4] + segs[-4:]}
        # step 3: full_model at the same threshold (the total norm is above every tensor's)
        tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=7)
        g3 = tr.flat("grad").copy()
        tr.set_solver(SolverOptions(clip_type="full_model", clip_value=max_norm))
        tr.apply_sgd(LR, MU, WD)
        out.update(n64_3=R.norms64(g3, inv, tab), norms3=tr.tensor("grad_norms").copy(), coef3=tr.tensor("clip_coef").copy())
        with pytest.raises(RsError):
            tr.set_solver(SolverOptions(clip_type="value", clip_value=0.0))
        tr.set_solver(SolverOptions(nesterov=True))
        with pytest.raises(RsError, match="momentum"):
            tr.apply_sgd(LR, 0.0, WD)                                      # Nesterov needs a momentum: refused by apply_sgd
        with pytest.raises(RsError):
            tr.grad_norms()                                                # this solver measures none
        yield out
    finally:
        tr.close()


def test_trainer_segment_table_is_the_buffer_in_order(assembled):
    segs = assembled["segs"]
    assert len(segs) > 40 and all(n.endswith(".w") != b for n, _, _, b in segs) and any(b for *_, b in segs)
    ends = [o + c for _, o, c, _ in segs]
    assert all(o % 4 == 0 for _, o, _, _ in segs) and all(o >= e for (_, o, _, _), e in zip(segs[1:], ends))
    assert any(o > e for (_, o, _, _), e in zip(segs[1:], ends))           # bias slots are 64-rounded: their padding lies in no segment


def test_trainer_without_a_solver_keeps_its_tensor_table(assembled):
    assert "grad_norms" not in assembled["names_unset"] and "clip_coef" not in assembled["names_unset"]
    assert assembled["names_set"] == assembled["names_unset"] + ["grad_norms", "clip_coef"]
    assert assembled["plain_step_is_the_restatement"] and not assembled["overflow1"] and not assembled["overflow2"]


def test_trainer_norms_and_coefficients_against_float64(assembled):
    n64, norms, coef, mx = assembled["n64"], assembled["norms"], assembled["coef"], assembled["max_norm"]
    rel = np.abs(norms - n64) / n64
    print(f"{assembled['precision']}: {len(n64)} tensors, norms {n64.min():.3e} .. {n64.max():.3e}, max_norm {mx:.3e}, worst norm error {rel.max() / R.U22:.3f} x 2^-22")
    assert (n64 > 0).all() and (rel <= R.U22).all()
    c64 = R.coef64(n64, mx)
    assert (coef == 1).sum() >= 5 and (coef < 1).sum() >= 5                # both branches
    assert (np.abs(coef - c64) <= R.U21 * c64).all()
    assert list(assembled["by_name"]) == [s[0] for s in assembled["segs"]] and np.array_equal(np.array(list(assembled["by_name"].values()), np.float32), norms)


def test_trainer_master_weights_after_the_clipped_nesterov_step(assembled):
    w64, _, tw, _ = assembled["want2"]
    err = np.abs(assembled["m2"] - w64)
    print(f"{assembled['precision']}: worst weight error / bound {(err / np.maximum(tw, 1e-300)).max():.3f}")
    assert (err <= tw).all()
    for (name, off, cnt, _) in assembled["segs"][:4] + assembled["segs"][-4:]:        # the "m:" tensors are those segments
        assert np.array_equal(assembled["m_tensors"][name].reshape(-1), assembled["m2"][off:off + cnt])


def test_trainer_full_model_has_one_coefficient(assembled):
    n64, coef = assembled["n64_3"], assembled["coef3"]
    c64 = R.coef64(R.total64(n64), assembled["max_norm"])
    assert (coef == coef[0]).all() and coef[0] < 1 and abs(coef[0] - c64) <= R.U21 * c64
    assert (np.abs(assembled["norms3"] - n64) <= R.U22 * n64).all()


def test_default_solver_and_no_solver_are_bit_identical(gpu_required):
    """set_solver(defaults) against never set: master weights after two steps, and after a third optimiser step on the same gradient
    (which reads the momentum the second left)."""
    spec = _spec(3, "fp16")
    Wn = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(2, 256, 256, 3, seed=777)
    gt_boxes, gt_classes, polys = _problem(3)
    got = []
    for solver in (None, SolverOptions()):
        tr = Trainer(spec, Wn, (256, 256, 3), batch=2, loss_scale=256.0, solver=solver)
        try:
            tr.set_sampling(256, 0.5, 64, 0.25)
            ms = []
            for it in range(2):
                tr.train_step(tiles, gt_boxes, gt_classes, polys, seed=5 + it)
                tr.apply_sgd(LR, MU, WD)
                ms.append(tr.flat("master").copy())
            tr.apply_sgd(LR, MU, WD)
            ms.append(tr.flat("master").copy())
            assert not tr.overflowed() and ("grad_norms" in tr.tensor_names()) == (solver is not None)
            got.append(ms)
        finally:
            tr.close()
    assert not np.array_equal(got[0][0], got[0][1]) and not np.array_equal(got[0][1], got[0][2])
    for a, b in zip(*got):
        assert np.array_equal(_bits(a), _bits(b))


def test_stem_padding_columns_hold_an_exactly_zero_gradient(gpu_required):
    """FREEZE_AT 0: the stem's [64][256] block has K = 147 real columns, (kh * 8 + kw) * 4 + ci with kw < 7 and ci < 3; a norm over the
    block is the tensor's norm only because every other column's gradient is exactly zero."""
    from tests.test_gpu_freeze_at import _spec as fa_spec
    spec = fa_spec("fp16", 3)
    tr = Trainer(spec, synthetic_weights(spec, seed=0), (256, 256, 3), batch=2, loss_scale=256.0, freeze_at=0)
    try:
        tr.set_sampling(256, 0.5, 64, 0.25)
        gt_boxes, _, polys = _problem(3)
        gt_classes = [np.array([0, 1, 0]), np.array([1, 0, 1, 0])]               # this spec has two classes
        tr.train_step(synthetic_tiles(2, 256, 256, 3, seed=777), gt_boxes, gt_classes, polys, seed=5)
        stem = [s for s in tr.segments() if "stem" in s[0]]
        assert [s[0].rsplit(".", 1)[1] for s in stem] == ["w"] and stem[0][2] == 64 * 256
        g = tr.tensor("g:" + stem[0][0])
        col = np.arange(256)
        real = ((col % 4) < 3) & ((col // 4) % 8 < 7) & (col // 32 < 7)
        assert real.sum() == 147 and g.shape == (64, 256)
        assert np.count_nonzero(g[:, real]) > 0.9 * 64 * 147 and not g[:, ~real].any()
    finally:
        tr.close()


# ------------------------------------------------------------------ the command line

def _run_cli(root, extra):
    import yaml
    from proj_roadsurf_amd import train_model
    from tests.test_gpu_trainer import _tiny_training_workdir
    root.mkdir()
    wd = _tiny_training_workdir(root)
    d2 = yaml.safe_load(open(root / "d2.yaml"))
    d2["TEST"]["EVAL_PERIOD"] = 0
    d2["SOLVER"]["CLIP_GRADIENTS"] = {"ENABLED": True, "CLIP_TYPE": "norm", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0}
    yaml.safe_dump(d2, open(root / "d2.yaml", "w"))
    cwd = os.getcwd()
    try:
        rc = train_model.main([str(root / "config.yaml"), "--synthetic-weights", "--log-period", "1", "--loss-scale", "256", "--precision", "fp16",
                               "--max-iter", "3", "--tagged-samples", "0"] + extra)
    finally:
        os.chdir(cwd)
    return rc, wd


def test_cli_trains_with_norm_clipping_under_the_switch_and_refuses_without(gpu_required, tmp_path):
    rc, wd = _run_cli(tmp_path / "extended", ["--solver", "extended"])
    recs = [json.loads(l) for l in open(wd / "logs" / "metrics.json")]
    assert rc == 0 and [r["iteration"] for r in recs] == [0, 1, 2]
    for r in recs:
        assert all(math.isfinite(r[k]) for k in ("total_loss", "loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")) and r["total_loss"] > 0
    with pytest.raises(SystemExit) as e:
        _run_cli(tmp_path / "default", [])
    assert "CLIP_GRADIENTS" in str(e.value) and "--solver extended" in str(e.value) and "unsupported training configuration" in str(e.value)
