"""Weight gradients of the fp32 trainer on split operands, the parts that need no GPU: the C ABI's new entries and their argument
checks, the host interface's refusals, the command line's switch, and the numpy statement of the arithmetic (tests/wgrad_split_ref.py)
against float64 inside the bound the GPU tests hold the kernel to."""
import ctypes as C
import os

import numpy as np
import pytest

from proj_roadsurf_amd.engine import MultiScaleTrainer, Trainer, WGRAD_MODES, load_library
from proj_roadsurf_amd.spec import EngineSpec
from tests import wgrad_split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rs_op_conv2d_wgrad_split", "rs_op_conv2d_wgrad_split_serves", "rs_trainer_set_wgrad_mode")
M, COUT, K = 1350, 32, 64


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
    geo = (2, 14, 14, 128, 1, 3, 3, 1, 1, 128, 9 * 128, 1, 0, None)
    assert lib.rs_op_conv2d_wgrad_split(None, None, None, None, *geo) < 0
    assert "rs_op_conv2d_wgrad_split" in err()
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)       # never read: the geometry below is refused first
    for bad in ((2, 14, 14, 100, 1, 3, 3, 1, 1, 128, 9 * 100, 1, 0, None),      # Cin no multiple of 64
                (2, 14, 14, 128, 0, 3, 3, 1, 1, 128, 9 * 128, 1, 0, None),      # input halo below the padding
                (2, 14, 14, 128, 1, 3, 3, 1, 1, 128, 9 * 128 + 64, 1, 0, None),  # padded K
                (0, 14, 14, 128, 1, 3, 3, 1, 1, 128, 9 * 128, 1, 0, None)):     # no image
        assert lib.rs_op_conv2d_wgrad_split(buf, buf, buf, None, *bad) < 0, bad
        assert "rs_op_conv2d_wgrad_split" in err(), err()
    assert lib.rs_trainer_set_wgrad_mode(None, 1) < 0
    assert "rs_trainer_set_wgrad_mode" in err()
    # every layer shape of the trainer is served; a channel count that is no multiple of 8 falls through to the fp32 kernel, and says so
    for cin, cout in ((256, 256), (64, 128), (512, 16), (12544, 1024), (1024, 256), (256, 64)):
        assert lib.rs_op_conv2d_wgrad_split_serves(cin, cout) == 1, (cin, cout)
    assert lib.rs_op_conv2d_wgrad_split_serves(256, 12) == 0


def test_host_interface_refuses_before_the_library_is_touched():
    assert WGRAD_MODES == ("f32", "split")
    spec = EngineSpec(num_classes=2, precision="fp32")
    with pytest.raises(ValueError, match="wgrad"):
        Trainer(spec, {}, (128, 128, 3), wgrad="gpu")
    with pytest.raises(ValueError, match="wgrad"):
        MultiScaleTrainer(spec, {}, (128, 128, 3), [128], wgrad="gpu")
    for cls, extra in ((Trainer, ()), (MultiScaleTrainer, ([128],))):
        with pytest.raises(ValueError, match="fp32 trainer"):
            cls(spec.replace(precision="fp16"), {}, (128, 128, 3), *extra, wgrad="split")
    ms = MultiScaleTrainer(spec, {}, (128, 128, 3), [128], wgrad="split")      # lazy: no trainer is built here
    assert ms.wgrad == "split"
    with pytest.raises(ValueError, match="wgrad"):
        ms.set_wgrad_mode("fp16")


def test_parser_takes_both_modes_and_defaults_to_f32():
    from proj_roadsurf_amd.train_model import build_parser
    ap = build_parser()
    assert ap.parse_args(["config.yaml"]).wgrad == "f32"
    for mode in WGRAD_MODES:
        assert ap.parse_args(["config.yaml", "--wgrad", mode]).wgrad == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["config.yaml", "--wgrad", "fp16"])


def test_exponent_puts_the_maximum_in_the_top_binade():
    rng = np.random.default_rng(0)
    for scale in (1e-30, 1e-7, 1.0, 3e3, 7e4, 1e20):
        a = (rng.standard_normal(1000) * scale).astype(np.float32)
        e = R.exponent(a)
        top = float(np.abs(np.ldexp(a, e)).max())
        assert 2.0 ** 14 <= top < 2.0 ** 15, (scale, e, top)
    assert R.exponent(np.zeros(8, np.float32)) == 0
    assert R.exponent(np.array([1.0, np.nan], np.float32)) == 0 and R.exponent(np.array([1.0, np.inf], np.float32)) == 0


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, name in enumerate(R.FAMILIES):
        dy, x = R.family(name, np.random.default_rng(100 + i), (M, COUT), (M, K))
        d64, x64 = dy.astype(np.float64), x.astype(np.float64)
        out[name] = (dy, x, d64.T @ x64, np.abs(d64).T @ np.abs(x64))
    return out


@pytest.mark.parametrize("name", R.FAMILIES)
def test_numpy_statement_stays_inside_the_bound(cases, name):
    dy, x, ref, S = cases[name]
    err = np.abs(R.wgrad_split(dy, x) - ref)
    lim = R.bound(S, M, np.abs(dy).max(), np.abs(x).max())
    used = float((err / lim).max())
    first_term_alone = float((err / (2.0 ** -20 * S)).max())
    print(f"{name}: largest error / bound {used:.3f}; against 2^-20 S alone {first_term_alone:.3f}")
    assert used <= 1.0, (name, used)
    if name == "heavy_tail":
        assert first_term_alone > 1.0       # the subnormal term of the bound is needed, not decoration


@pytest.mark.parametrize("name", R.FAMILIES)
def test_planes_do_not_depend_on_a_power_of_two_factor(cases, name):
    dy, x, _, _ = cases[name]
    for a in (dy, x):
        b = np.ldexp(a, -30).astype(np.float32)
        ea, eb = R.exponent(a), R.exponent(b)
        assert eb == ea + 30
        for p, q in zip(R.planes(a, ea), R.planes(b, eb)):
            assert np.array_equal(p.view(np.uint16), q.view(np.uint16))
