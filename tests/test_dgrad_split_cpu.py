"""Input gradients of the fp32 trainer on split operands, the parts that need no GPU: the C ABI's new entries and their argument checks,
the host interface's refusals, the command line's switch, and the numpy statement of the arithmetic (tests/dgrad_split_ref.py) against
float64 inside the bound the GPU tests hold the kernel to."""
import ctypes as C
import os

import numpy as np
import pytest

from proj_roadsurf_amd import engine as E
from proj_roadsurf_amd.engine import MultiScaleTrainer, Trainer, load_library
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import split_planes
from tests import dgrad_split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_conv2d_dgrad_split", "rs_op_conv2d_dgrad_split_serves", "rs_op_split_rows", "rs_trainer_set_dgrad_mode")
M, ROWS, T = 300, 48, 9 * 64

# (cin, K side = cout padded to 64, k, stride) of every add_dgrad stage of the model: FPN outputs / RPN conv / mask convs, the laterals,
# conv3 / conv2 / conv1 / shortcut of res3 - res5 (STRIDE_IN_1X1), the RPN heads and the two predictors (16 rows padded to 64), fc2, fc1
MODEL_SHAPES = ([(256, 256, 3, 1)] + [(c, 256, 1, 1) for c in (256, 512, 1024, 2048)] +
                [(128, 512, 1, 1), (256, 1024, 1, 1), (512, 2048, 1, 1), (128, 128, 3, 1), (256, 256, 3, 1), (512, 512, 3, 1),
                 (256, 128, 1, 2), (512, 128, 1, 1), (512, 256, 1, 2), (1024, 256, 1, 1), (1024, 512, 1, 2), (2048, 512, 1, 1),
                 (256, 512, 1, 2), (512, 1024, 1, 2), (1024, 2048, 1, 2),
                 (256, 64, 1, 1), (1024, 64, 1, 1), (1024, 1024, 1, 1), (12544, 1024, 1, 1)])


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
    # n, hi, wi, cin, ho, wo, cout, kh, kw, stride, pad, kpad, halo, variant, count, stream
    good = (2, 14, 14, 64, 14, 14, 128, 3, 3, 1, 1, 9 * 128, 1, -1, None, None)
    assert lib.rs_op_conv2d_dgrad_split(None, None, None, None, None, None, None, *good) < 0
    assert "rs_op_conv2d_dgrad_split" in err()
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)       # never read: the arguments below are refused first
    for what, bad in (("K side no multiple of 64", (2, 14, 14, 64, 14, 14, 100, 3, 3, 1, 1, 9 * 128, 1, -1, None, None)),
                      ("stride 2 with a 3x3 kernel", (2, 14, 14, 64, 7, 7, 128, 3, 3, 2, 1, 9 * 128, 1, -1, None, None)),
                      ("halo below k - 1 - pad", (2, 14, 14, 64, 14, 14, 128, 3, 3, 1, 1, 9 * 128, 0, -1, None, None)),
                      ("no image", (0, 14, 14, 64, 14, 14, 128, 3, 3, 1, 1, 9 * 128, 1, -1, None, None))):
        assert lib.rs_op_conv2d_dgrad_split(buf, buf, buf, None, None, None, None, *bad) < 0, what
        assert "rs_op_conv2d_dgrad_split" in err(), (what, err())
    assert lib.rs_op_conv2d_dgrad_split(buf, None, buf, None, None, None, None, *good) < 0 and "null" in err()
    assert lib.rs_op_split_rows(None, 4, 64, None, None, None) < 0
    assert "rs_op_split_rows" in err()
    assert lib.rs_trainer_set_dgrad_mode(None, 1) < 0
    assert "rs_trainer_set_dgrad_mode" in err()


def test_every_stage_shape_of_the_model_is_served():
    lib = load_library()
    for cin, cout, k, stride in MODEL_SHAPES:
        assert lib.rs_op_conv2d_dgrad_split_serves(cin, cout, k, stride) == 1, (cin, cout, k, stride)
    assert lib.rs_op_conv2d_dgrad_split_serves(256, 16, 1, 1) == 0          # the K side must arrive padded to 64
    assert lib.rs_op_conv2d_dgrad_split_serves(256, 96, 3, 1) == 0
    assert lib.rs_op_conv2d_dgrad_split_serves(256, 128, 3, 2) == 0         # a strided 3x3 is not an input gradient this network has


def test_host_interface_refuses_before_the_library_is_touched():
    assert E.DGRAD_MODES == ("f32", "split")
    assert E.WGRAD_MODES == ("f32", "split")
    spec = EngineSpec(num_classes=2, precision="fp32")
    with pytest.raises(ValueError, match="dgrad"):
        Trainer(spec, {}, (128, 128, 3), dgrad="gpu")
    with pytest.raises(ValueError, match="dgrad"):
        MultiScaleTrainer(spec, {}, (128, 128, 3), [128], dgrad="gpu")
    for cls, extra in ((Trainer, ()), (MultiScaleTrainer, ([128],))):
        with pytest.raises(ValueError, match="fp32 trainer"):
            cls(spec.replace(precision="fp16"), {}, (128, 128, 3), *extra, dgrad="split")
    ms = MultiScaleTrainer(spec, {}, (128, 128, 3), [128], dgrad="split")      # lazy: no trainer is built here
    assert ms.dgrad == "split" and ms.wgrad == "f32"
    with pytest.raises(ValueError, match="dgrad"):
        ms.set_dgrad_mode("fp16")


def test_parser_takes_both_modes_and_defaults_to_f32():
    from proj_roadsurf_amd.train_model import build_parser
    ap = build_parser()
    assert ap.parse_args(["config.yaml"]).dgrad == "f32"
    for mode in E.DGRAD_MODES:
        assert ap.parse_args(["config.yaml", "--dgrad", mode]).dgrad == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["config.yaml", "--dgrad", "fp16"])


def test_row_planes_are_weights_split_planes():
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((96, 576)) * np.exp2(rng.uniform(-20, 20, (96, 1)))).astype(np.float32)
    w[5] = 0
    w[17] = 1e-30
    hi, lo, inv, e = R.row_planes(w)
    want_planes, want_inv = split_planes(w)
    assert np.array_equal(np.concatenate([hi, lo], 0).view(np.uint16), want_planes.view(np.uint16))
    assert np.array_equal(inv.view(np.uint32), want_inv.view(np.uint32))
    top = np.abs(np.ldexp(w.astype(np.float64), e[:, None])).max(axis=1)
    ordinary = np.ones(96, bool)
    ordinary[[5, 17]] = False
    assert ((top[ordinary] >= 2.0 ** 13) & (top[ordinary] < 2.0 ** 14)).all()
    assert e[5] == 0 and e[17] == 100 and inv[5] == 1.0


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, name in enumerate(R.FAMILIES):
        dy, w = R.family(name, np.random.default_rng(200 + i), (M, T), (ROWS, T))
        d64, w64 = dy.astype(np.float64), w.astype(np.float64)
        out[name] = (dy, w, d64 @ w64.T, np.abs(d64) @ np.abs(w64).T)
    return out


@pytest.mark.parametrize("name", R.FAMILIES)
def test_numpy_statement_stays_inside_the_bound(cases, name):
    dy, w, ref, S = cases[name]
    err = np.abs(R.dgrad_split(dy, w) - ref)
    lim = R.bound(S, T, np.abs(dy).max(), np.abs(w).max(axis=1))
    used = float((err / lim).max())
    first_term_alone = float((err / (2.0 ** -20 * S)).max())
    print(f"{name}: largest error / bound {used:.3f}; against 2^-20 S alone {first_term_alone:.3f}")
    assert used <= 1.0, (name, used)
    if name == "heavy_tail":
        assert first_term_alone > 1.0       # the sub-normal-range term of the bound is needed, not decoration


@pytest.mark.parametrize("name", R.FAMILIES)
def test_planes_and_row_scales_do_not_depend_on_a_power_of_two_factor(cases, name):
    dy, w, _, _ = cases[name]
    b = np.ldexp(dy, -30).astype(np.float32)
    ea, eb = R.exponent(dy), R.exponent(b)
    assert eb == ea + 30
    for p, q in zip(R.planes(dy, ea), R.planes(b, eb)):
        assert np.array_equal(p.view(np.uint16), q.view(np.uint16))
    hi, lo, inv, e = R.row_planes(w)
    hi2, lo2, inv2, e2 = R.row_planes(np.ldexp(w, 10).astype(np.float32))
    assert np.array_equal(e2, e - 10)
    assert np.array_equal(hi.view(np.uint16), hi2.view(np.uint16)) and np.array_equal(lo.view(np.uint16), lo2.view(np.uint16))
    assert np.array_equal(np.ldexp(inv, 10).view(np.uint32), inv2.view(np.uint32))
    got, scaled = R.dgrad_split(dy, w), R.dgrad_split(b, np.ldexp(w, 10).astype(np.float32))
    assert np.array_equal(np.ldexp(got, -20), scaled)
