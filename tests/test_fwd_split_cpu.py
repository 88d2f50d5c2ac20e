"""Forward pass of the fp32 trainer on split operands, the parts that need no GPU: the C ABI's new entries and their argument checks,
the host interface's refusals, the command line's switch, and the numpy statement of the arithmetic against float64 inside the bound
the GPU tests hold the kernel to.  The product is the input gradient's with x in dY's role (tests/dgrad_split_ref.py); the forward
epilogue -- bias, res, up, ReLU in fp32 -- is `epilogue` below."""
import ctypes as C
import os

import numpy as np
import pytest

from proj_roadsurf_amd import engine as E
from proj_roadsurf_amd.engine import MultiScaleTrainer, Trainer, load_library
from proj_roadsurf_amd.spec import EngineSpec
from tests import dgrad_split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_conv2d_fwd_split", "rs_op_conv2d_fwd_split_serves", "rs_trainer_set_fwd_mode")
M, ROWS, T = 300, 48, 9 * 64

# (cin, cout, k, stride) of every forward conv / linear stage of the model under the reference YAML (STRIDE_IN_1X1: the first block of
# res3 / res4 / res5 strides in conv1 and in the shortcut)
RES2 = [(64, 64, 1, 1), (64, 64, 3, 1), (64, 256, 1, 1), (256, 64, 1, 1)]
RES345 = [s for cin, b in ((256, 128), (512, 256), (1024, 512)) for s in
          ((cin, b, 1, 2), (4 * b, b, 1, 1), (b, b, 3, 1), (b, 4 * b, 1, 1), (cin, 4 * b, 1, 2))]
LATERALS = [(c, 256, 1, 1) for c in (256, 512, 1024, 2048)]
HEADS = [(256, 256, 3, 1),                         # FPN outputs, the RPN conv, the mask convs
         (256, 16, 1, 1), (1024, 16, 1, 1),        # the RPN head and the mask predictor; the box predictor
         (12544, 1024, 1, 1), (1024, 1024, 1, 1)]  # fc1, fc2
MODEL_SHAPES = RES2 + RES345 + LATERALS + HEADS


def epilogue(gemm, bias, res=None, up=None, relu=False):
    """The forward epilogue in fp32 on a gemm [n][h][w][c] (any float type): + bias [c], + res (gemm's shape), + up [n][ceil(h/2)][ceil(w/2)][c]
    at (y >> 1, x >> 1), ReLU -- ref_f32.hip's order."""
    v = np.asarray(gemm, np.float32) + np.asarray(bias, np.float32)
    if res is not None:
        v = v + np.asarray(res, np.float32)
    if up is not None:
        n, h, w, c = v.shape
        v = v + np.asarray(up, np.float32).repeat(2, axis=1).repeat(2, axis=2)[:, :h, :w]
    return np.maximum(v, np.float32(0)) if relu else v


def test_header_declares_and_library_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "rs_engine.h")).read()
    lib = load_library()
    for name in ENTRIES:
        assert f"int {name}(" in hdr, name
        assert hasattr(lib, name), name
    assert lib.rs_abi_version() == 1


def test_entries_refuse_bad_arguments_before_touching_a_device():
    """No GPU here: a call that got past its argument checks would fail with a HIP error instead of these messages."""
    lib = load_library()
    err = lambda: lib.rs_last_error().decode()
    # n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, out_halo, relu, variant, count, stream
    good = (2, 14, 14, 64, 1, 3, 3, 1, 1, 128, 9 * 64, 1, 0, -1, None, None)
    assert lib.rs_op_conv2d_fwd_split(None, None, None, None, None, None, *good) < 0
    assert "rs_op_conv2d_fwd_split" in err() and "null" in err()
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)       # never read: the arguments below are refused first
    for what, bad in (("no image", (0, 14, 14, 64, 1, 3, 3, 1, 1, 128, 9 * 64, 1, 0, -1, None, None)),
                      ("K side 100", (2, 14, 14, 100, 1, 3, 3, 1, 1, 128, 9 * 128, 1, 0, -1, None, None)),
                      ("rows 24", (2, 14, 14, 64, 1, 3, 3, 1, 1, 24, 9 * 64, 1, 0, -1, None, None)),
                      ("halo below the pad", (2, 14, 14, 64, 0, 3, 3, 1, 1, 128, 9 * 64, 1, 0, -1, None, None)),
                      ("kpad below kh kw cin", (2, 14, 14, 64, 1, 3, 3, 1, 1, 128, 8 * 64, 1, 0, -1, None, None))):
        assert lib.rs_op_conv2d_fwd_split(buf, buf, buf, buf, None, None, *bad) == -1, what
        assert "rs_op_conv2d_fwd_split" in err(), (what, err())
    for i in range(4):                                               # x, w, bias, y: each alone is refused as null
        ops = [buf] * 4
        ops[i] = None
        assert lib.rs_op_conv2d_fwd_split(*ops, None, None, *good) < 0 and "null" in err(), i
    assert lib.rs_trainer_set_fwd_mode(None, 1) < 0
    assert "rs_trainer_set_fwd_mode" in err()


def test_every_forward_stage_shape_of_the_model_is_served():
    lib = load_library()
    assert len(MODEL_SHAPES) == 4 + 15 + 4 + 5
    for cin, cout, k, stride in MODEL_SHAPES:
        assert lib.rs_op_conv2d_fwd_split_serves(cin, cout, k, stride) == 1, (cin, cout, k, stride)
    assert lib.rs_op_conv2d_fwd_split_serves(4, 64, 7, 2) == 0          # the stem
    assert lib.rs_op_conv2d_fwd_split_serves(3, 64, 7, 2) == 0
    assert lib.rs_op_conv2d_fwd_split_serves(96, 128, 3, 1) == 0
    assert lib.rs_op_conv2d_fwd_split_serves(64, 24, 1, 1) == 0
    assert lib.rs_op_conv2d_dgrad_split_serves(256, 128, 3, 2) == 0     # the input gradient's own rule still answers as it did


def test_host_interface_refuses_before_the_library_is_touched():
    assert E.FWD_MODES == ("f32", "split")
    assert E.DGRAD_MODES == E.WGRAD_MODES == ("f32", "split")
    spec = EngineSpec(num_classes=2, precision="fp32")
    with pytest.raises(ValueError, match="fwd"):
        Trainer(spec, {}, (128, 128, 3), fwd="gpu")
    with pytest.raises(ValueError, match="fwd"):
        MultiScaleTrainer(spec, {}, (128, 128, 3), [128], fwd="gpu")
    for cls, extra in ((Trainer, ()), (MultiScaleTrainer, ([128],))):
        with pytest.raises(ValueError, match="fp32 trainer"):
            cls(spec.replace(precision="fp16"), {}, (128, 128, 3), *extra, fwd="split")
    ms = MultiScaleTrainer(spec, {}, (128, 128, 3), [128], fwd="split")      # lazy: no trainer is built here
    assert ms.fwd == "split" and ms.wgrad == "f32" and ms.dgrad == "f32"
    with pytest.raises(ValueError, match="fwd"):
        ms.set_fwd_mode("fp16")
    with pytest.raises(ValueError, match="fp32 trainer"):
        MultiScaleTrainer(spec.replace(precision="fp16"), {}, (128, 128, 3), [128]).set_fwd_mode("split")


def test_parser_takes_both_modes_and_defaults_to_f32():
    from proj_roadsurf_amd.train_model import build_parser
    ap = build_parser()
    assert ap.parse_args(["config.yaml"]).fwd == "f32"
    for mode in E.FWD_MODES:
        assert ap.parse_args(["config.yaml", "--fwd", mode]).fwd == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["config.yaml", "--fwd", "fp16"])


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, name in enumerate(R.FAMILIES):
        x, w = R.family(name, np.random.default_rng(300 + i), (M, T), (ROWS, T))
        x64, w64 = x.astype(np.float64), w.astype(np.float64)
        out[name] = (x, w, x64 @ w64.T, np.abs(x64) @ np.abs(w64).T)
    return out


@pytest.mark.parametrize("name", R.FAMILIES)
def test_numpy_statement_stays_inside_the_bound(cases, name):
    x, w, ref, S = cases[name]
    err = np.abs(R.dgrad_split(x, w) - ref)
    lim = R.bound(S, T, np.abs(x).max(), np.abs(w).max(axis=1))
    used = float((err / lim).max())
    print(f"{name}: largest error / bound {used:.3f}")
    assert used <= 1.0, (name, used)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_numpy_statement_with_the_forward_epilogue_stays_inside_the_bound(cases, name):
    """M = 300 rows as a 1 x 15 x 20 image: bias, res, up from the 8 x 10 coarser map, ReLU -- against the same in float64."""
    x, w, ref, S = cases[name]
    rng = np.random.default_rng(77)
    shape = (1, 15, 20, ROWS)
    bias = rng.standard_normal(ROWS).astype(np.float32)
    res = rng.standard_normal(shape).astype(np.float32)
    up = rng.standard_normal((1, 8, 10, ROWS)).astype(np.float32)
    up_full = up.repeat(2, axis=1).repeat(2, axis=2)[:, :15, :20]
    got = epilogue(R.dgrad_split(x, w).reshape(shape), bias, res, up, relu=True)
    want = np.maximum(ref.reshape(shape) + bias.astype(np.float64) + res + up_full, 0.0)
    adds = np.abs(bias.astype(np.float64)) + np.abs(res) + np.abs(up_full)
    lim = R.bound(S, T, np.abs(x).max(), np.abs(w).max(axis=1)).reshape(shape) + R.epilogue_allowance(ref.reshape(shape), adds)
    used = float((np.abs(got - want) / lim).max())
    print(f"{name} + bias + res + up + relu: largest error / bound {used:.3f}")
    assert used <= 1.0, (name, used)
    assert (got == 0).any() and (got > 0).any()
    plain = epilogue(ref.reshape(shape), np.zeros(ROWS, np.float32))
    assert np.array_equal(plain, ref.reshape(shape).astype(np.float32))      # zero bias, no addend, no ReLU: the product alone
