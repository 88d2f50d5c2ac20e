"""torchvision's batched_nms size rule (EngineSpec.batched_nms = "torchvision") without a GPU: the statement the GPU tests
use as their reference -- one NMS per category on shifted coordinates == torchvision's single NMS over all shifted boxes --
against the oracle, and the option's way from EngineSpec and the CLIs to rs_spec."""
import ctypes as C
import os

import numpy as np
import pytest

from proj_roadsurf_amd.engine import LIB_PATH, RS_SPEC_SIZE_V1, RsSpec, load_library, make_rs_spec
from proj_roadsurf_amd.spec import BATCHED_NMS_MODES, EngineSpec
from tests import batched_nms_ref as R


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return load_library()


# ------------------------------------------------------------------ the layout claim
@pytest.mark.parametrize("t", [0.5, 0.7])
@pytest.mark.parametrize("G", [2, 5, 8])
def test_per_category_nms_on_shifted_boxes_equals_torchvisions_single_nms(G, t):
    """rule_keep (category g alone on boxes + fl(g * fl(max + 1))) == oracle.batched_nms(coordinate_trick=True), flag for flag,
    on seeded images of near-threshold pairs with a box from coordinate 0, a box up to the largest coordinate, the threshold
    pairs of tests/util.py and invalid entries; and the fixture is one on which that differs from per-category arithmetic."""
    differ = 0
    for seed in range(3):
        rng = np.random.default_rng(1000 * G + int(t * 10) + seed)
        boxes, valid, counts = R.make_image(rng, G, 1024, t, R.spread(800, list(range(G)), G), invalid=5)
        assert valid[np.arange(1024)[None, :] < counts[:, None]].min() == 0 and boxes.min() == 0.0
        got, taken, unit, total = R.rule_keep(boxes, valid, counts, t)
        assert taken and total == int(sum(valid[g, :counts[g]].sum() for g in range(G))) < int(counts.sum())
        assert float(unit) == float(np.float32(np.float32(boxes.max()) + np.float32(1)))
        want = R.oracle_keep(boxes, valid, counts, t, coordinate_trick=True)
        assert np.array_equal(got, want), (G, t, seed, np.argwhere(got != want)[:8])
        plain = R.oracle_keep(boxes, valid, counts, t, coordinate_trick=False)
        assert np.array_equal(plain, R.category_keep(boxes, valid, counts, t))
        assert not plain[valid == 0].any() and not want[valid == 0].any()
        differ += int((plain != want).sum())
    assert differ >= 8, f"{G} categories, t {t}: the two branches differ in {differ} flags only"


def test_rule_decision_thresholds():
    """taken for 1 .. 1000 boxes, not for 0 or 1001; invalid entries do not count; the oracle's own size rule agrees."""
    rng = np.random.default_rng(5)
    for total, want in ((0, False), (1, True), (1000, True), (1001, False)):
        b, v, c = R.make_image(rng, 5, 1024, 0.7, R.spread(total, [0, 1, 2, 3, 4], 5), touch_border=False)
        assert R.rule_decision(b, v, c)[0] is want and R.rule_decision(b, v, c)[2] == total
        keep = R.rule_keep(b, v, c, 0.7)[0]
        assert np.array_equal(keep, R.oracle_keep(b, v, c, 0.7, coordinate_trick=None)), total
    b, v, c = R.operator_fixture(2, 1024, 0.5, 1, [("invalid", 1100, 150, [0, 1])])
    assert int(c[0].sum()) == 1100 and R.rule_decision(b[0], v[0], c[0])[0] and R.rule_decision(b[0], v[0], c[0])[2] == 950
    assert np.array_equal(R.rule_keep(b[0], v[0], c[0], 0.5)[0], R.oracle_keep(b[0], v[0], c[0], 0.5, coordinate_trick=None))


# ------------------------------------------------------------------ the option
def test_engine_spec_batched_nms_default_and_validation():
    assert EngineSpec().batched_nms == "per_category" == BATCHED_NMS_MODES[0]
    assert EngineSpec(batched_nms="torchvision").batched_nms == "torchvision"
    assert EngineSpec().replace(batched_nms="torchvision").replace(num_classes=3).batched_nms == "torchvision"
    for bad in ("tv", "per-category", "", None, 1):
        with pytest.raises(ValueError):
            EngineSpec(batched_nms=bad)
    with pytest.raises(ValueError):
        EngineSpec().replace(batched_nms="coordinate_trick")


def test_make_rs_spec_round_trip_and_old_struct_size(lib):
    """make_rs_spec writes the mode behind every earlier field; the library reads a block of the earlier size as mode off,
    the current size as the field says, and rejects every other size and value."""
    off = make_rs_spec(EngineSpec(num_classes=2))
    on = make_rs_spec(EngineSpec(num_classes=2, batched_nms="torchvision"))
    assert off.batched_nms == 0 and on.batched_nms == 1
    assert off.struct_size == on.struct_size == C.sizeof(RsSpec) == RS_SPEC_SIZE_V1 + 4
    assert RsSpec.batched_nms.offset == RsSpec.precision.offset + 4                    # appended: no earlier field moved
    assert bytes(off)[:RS_SPEC_SIZE_V1] == bytes(on)[:RS_SPEC_SIZE_V1]
    assert lib.rs_spec_batched_nms(C.byref(off)) == 0 and lib.rs_spec_batched_nms(C.byref(on)) == 1
    old = make_rs_spec(EngineSpec(num_classes=2, batched_nms="torchvision"))
    old.struct_size = RS_SPEC_SIZE_V1                                                  # a caller built against the earlier header
    assert lib.rs_spec_batched_nms(C.byref(old)) == 0
    for size in (RS_SPEC_SIZE_V1 - 4, RS_SPEC_SIZE_V1 + 8, 0):
        bad = make_rs_spec(EngineSpec(num_classes=2))
        bad.struct_size = size
        assert lib.rs_spec_batched_nms(C.byref(bad)) < 0
        assert b"size mismatch" in lib.rs_last_error()
    bad = make_rs_spec(EngineSpec(num_classes=2))
    bad.batched_nms = 2
    assert lib.rs_spec_batched_nms(C.byref(bad)) < 0


def test_cli_option_parses():
    from proj_roadsurf_amd import make_detections, train_model
    for mod in (make_detections, train_model):
        ap = mod.build_parser()
        assert ap.parse_args(["cfg.yaml"]).batched_nms == "per-category"
        assert ap.parse_args(["cfg.yaml", "--batched-nms", "torchvision"]).batched_nms == "torchvision"
        assert ap.parse_args(["cfg.yaml", "--batched-nms", "per-category"]).batched_nms == "per-category"
        with pytest.raises(SystemExit):
            ap.parse_args(["cfg.yaml", "--batched-nms", "coordinate-trick"])
        assert EngineSpec(batched_nms=ap.parse_args(["cfg.yaml", "--batched-nms", "torchvision"]).batched_nms.replace("-", "_"))

