"""Training diagnostics without a GPU: the host restatements of csrc/train_stats.h (the header the three kernels include) against the
numpy reference, exactly; the arithmetic of the scalars and detectron2's omission rules; the refusals of the C entries; the CLI
switch."""
import ctypes as C

import numpy as np
import pytest

from proj_roadsurf_amd import engine as E
from proj_roadsurf_amd.engine import load_library
from tests import train_stats_ref as R
from tests.train_stats_cases import DENORM, box_cases, label_cases, mask_cases


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _buf(a, dtype):
    """A contiguous array of at least one element (an empty case still hands the entry a real pointer)."""
    a = np.ascontiguousarray(a, dtype)
    return a if a.size else np.zeros(1, dtype)


@pytest.fixture(scope="module")
def lib():
    return load_library()


@pytest.fixture(scope="module")
def codes():
    """The error codes as csrc/common.h defines them."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "proj_roadsurf_amd", "csrc", "common.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(RS_ERR_[A-Z]+)\s+(-?\d+)", hdr)}


def host_label_counts(lib, labels, start=(0, 0)):
    out = np.array(start, np.int32)
    l = _buf(labels, np.int32)
    assert lib.rs_host_label_counts(_p(l), len(labels), _p(out)) == 0, lib.rs_last_error()
    return out


def host_box_stats(lib, c, start=None):
    out = np.zeros(7, np.int32) if start is None else np.array(start, np.int32)
    sc = c["sampled"]
    rc = lib.rs_host_box_stats(_p(c["pred"]), _p(c["cls"]), len(c["cls"]), c["K"], c["cs"], _p(sc) if sc is not None else None,
                               0 if sc is None else len(sc), _p(out))
    assert rc == 0, lib.rs_last_error()
    return out


def host_mask_stats(lib, c):
    out = np.zeros(5, np.int32)
    ptr = None if c["ptr"] is None else np.array([c["ptr"]], np.int32)
    lg, tg, cl = _buf(c["logits"], np.float32), _buf(c["targets"], np.uint8), _buf(c["cls"], np.int32)
    rc = lib.rs_host_mask_stats(_p(lg), _p(tg), _p(cl), _p(ptr) if ptr is not None else None, c["n_masks"], c["side"], c["cs"], _p(out))
    assert rc == 0, lib.rs_last_error()
    return out


@pytest.mark.parametrize("case", label_cases(), ids=lambda c: c["name"])
def test_host_label_counts_equal_numpy(lib, case):
    assert np.array_equal(host_label_counts(lib, case["labels"]), R.label_counts(case["labels"]))


@pytest.mark.parametrize("case", box_cases(), ids=lambda c: c["name"])
def test_host_box_stats_equal_numpy(lib, case):
    want = R.box_stats(case["pred"], case["cls"], case["K"], case["sampled"])
    assert np.array_equal(host_box_stats(lib, case), want), (case["name"], want)


def test_box_cases_pin_what_they_name():
    """The hand-made rows give the counts their names promise (inst, correct, fgn, fg_correct, fg_as_bg), so that a reference which
    broke ties towards the last index, or read a delta column, would not pass unnoticed."""
    by = {c["name"]: R.box_stats(c["pred"], c["cls"], c["K"], c["sampled"])[2:].tolist() for c in box_cases()}
    assert by["ties-first-index-wins"] == [4, 2, 3, 2, 0]        # preds 0, 0, 1, 1 against classes 0, 2, 1, 3
    assert by["signed-zeros-tie"] == [3, 1, 2, 1, 0]             # preds 0, 0, 1 against classes 0, 1, 3
    assert by["maximum-in-the-last-logit"] == [5, 1, 4, 0, 4]    # every row predicts background
    assert by["all-empty"] == [0, 0, 0, 0, 0] and by["labels-minus2-and-K+1-ignored"] == [0, 0, 0, 0, 0]
    assert by["all-background"][0] == 257 and by["all-background"][2] == 0
    assert by["all-foreground"][0] == 257 and by["all-foreground"][2] == 257
    assert by["infinities"] == [3, 2, 3, 2, 0]                   # preds 0, 1, 1 against classes 0, 2, 1


@pytest.mark.parametrize("case", mask_cases(), ids=lambda c: c["name"])
def test_host_mask_stats_equal_numpy(lib, case):
    want = R.mask_stats(case["logits"], case["targets"], case["cls"], case["ptr"])
    assert np.array_equal(host_mask_stats(lib, case), want), (case["name"], want)


def test_positive_predicate_answers_as_ieee(lib):
    """+0.0, -0.0 false; the smallest denormal and +inf true; their negatives false -- one pixel each, target 0, so that false_pos
    counts exactly the logits that are > 0."""
    vals = np.array([0.0, -0.0, DENORM, -DENORM, 1e-30, -1e-30, np.inf, -np.inf], np.float32)
    for v, want in zip(vals, (0, 0, 1, 0, 1, 0, 1, 0)):
        c = dict(logits=np.full((1, 1, 1), v, np.float32), targets=np.zeros((1, 1), np.uint8), cls=np.zeros(1, np.int32), ptr=None, side=1, cs=1, n_masks=1)
        assert host_mask_stats(lib, c).tolist() == [1, want, 0, want, 0], float(v)


def test_host_entries_add_into_the_counts(lib):
    c = box_cases()[4]
    once = host_box_stats(lib, c)
    assert np.array_equal(host_box_stats(lib, c, start=once), 2 * once)
    l = label_cases()[2]["labels"]
    assert np.array_equal(host_label_counts(lib, l, start=(5, 7)), R.label_counts(l) + [5, 7])


def _table(**kw):
    t = np.zeros(16, np.int32)
    names = ("pos", "neg", "fg", "bg", "inst", "correct", "fgn", "fg_correct", "fg_as_bg", "pixels", "incorrect", "positive", "false_pos", "false_neg", "n")
    for k, v in kw.items():
        t[names.index(k)] = v
    return t


def test_scalars_carry_detectron2s_names_and_arithmetic():
    t = _table(pos=30, neg=226, fg=50, bg=206, inst=256, correct=200, fgn=50, fg_correct=10, fg_as_bg=35, pixels=39200, incorrect=9800,
               positive=20000, false_pos=4800, false_neg=5000, n=2)
    s = E.train_stats_scalars(t)
    assert tuple(s) == E.TRAIN_STATS_KEYS
    assert s == {"rpn/num_pos_anchors": 15.0, "rpn/num_neg_anchors": 113.0, "roi_head/num_fg_samples": 25.0, "roi_head/num_bg_samples": 103.0,
                 "fast_rcnn/cls_accuracy": 200 / 256, "fast_rcnn/fg_cls_accuracy": 10 / 50, "fast_rcnn/false_negative": 35 / 50,
                 "mask_rcnn/accuracy": 1.0 - 9800 / 39200, "mask_rcnn/false_positive": 4800 / 19200, "mask_rcnn/false_negative": 5000 / 20000}
    assert all(type(v) is float for v in s.values())
    assert E.train_stats_scalars(t.tolist()) == s


def test_scalars_omit_what_detectron2_omits():
    box = {"fast_rcnn/cls_accuracy", "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative"}
    mask = {"mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative"}
    full = dict(pos=3, neg=5, fg=4, bg=12, inst=16, correct=9, fgn=4, fg_correct=1, fg_as_bg=2, pixels=784, incorrect=100, positive=300,
                false_pos=40, false_neg=60, n=1)
    assert set(E.train_stats_scalars(_table(**full))) == set(E.TRAIN_STATS_KEYS)
    no_inst = dict(full, inst=0, correct=0, fgn=0, fg_correct=0, fg_as_bg=0)
    assert set(E.train_stats_scalars(_table(**no_inst))) == set(E.TRAIN_STATS_KEYS) - box
    no_fg = dict(full, fgn=0, fg_correct=0, fg_as_bg=0)                       # a batch of background RoIs only
    assert set(E.train_stats_scalars(_table(**no_fg))) == set(E.TRAIN_STATS_KEYS) - box | {"fast_rcnn/cls_accuracy"}
    no_mask = dict(full, pixels=0, incorrect=0, positive=0, false_pos=0, false_neg=0)      # no entries, or MASK_ON false: mask.stats never ran
    assert set(E.train_stats_scalars(_table(**no_mask))) == set(E.TRAIN_STATS_KEYS) - mask
    with pytest.raises(ValueError):
        E.train_stats_scalars(np.zeros(15, np.int32))


def test_scalars_keep_their_denominators_at_one_or_more():
    """Every target pixel set: false_positive divides by max(pixels - positive, 1) = 1.  None set: false_negative by max(positive, 1)."""
    s = E.train_stats_scalars(_table(n=1, pixels=784, incorrect=84, positive=784, false_pos=0, false_neg=84))
    assert s["mask_rcnn/false_positive"] == 0.0 and s["mask_rcnn/false_negative"] == 84 / 784 and s["mask_rcnn/accuracy"] == 1.0 - 84 / 784
    s = E.train_stats_scalars(_table(n=1, pixels=784, incorrect=10, positive=0, false_pos=10, false_neg=0))
    assert s["mask_rcnn/false_negative"] == 0.0 and s["mask_rcnn/false_positive"] == 10 / 784


def test_entries_refuse_bad_arguments_before_touching_a_device(lib, codes):
    """No GPU here: a refusal that came after a device call would be a HIP error, not RS_ERR_ARG with the entry's name."""
    arg, uns = codes["RS_ERR_ARG"], codes["RS_ERR_UNSUPPORTED"]
    f, i, u, o = np.zeros(64, np.float32), np.zeros(4, np.int32), np.zeros(4, np.uint8), np.zeros(8, np.int32)
    for fam in ("op", "host"):
        tail = (None,) if fam == "op" else ()
        lc, bs, ms = (getattr(lib, f"rs_{fam}_{n}") for n in ("label_counts", "box_stats", "mask_stats"))

        def refused(rc, want, name):
            assert rc == want, (name, rc, lib.rs_last_error())
            assert f"rs_{fam}_{name}".encode() in lib.rs_last_error()
        refused(lc(None, 4, _p(o), *tail), arg, "label_counts")
        refused(lc(_p(i), 4, None, *tail), arg, "label_counts")
        refused(lc(_p(i), -1, _p(o), *tail), arg, "label_counts")
        refused(lc(_p(i), 1 << 31, _p(o), *tail), uns, "label_counts")
        refused(bs(None, _p(i), 4, 3, 16, None, 0, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), None, 4, 3, 16, None, 0, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), 4, 3, 16, None, 0, None, *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), -1, 3, 16, None, 0, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), 4, 3, 16, None, -1, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), 4, 0, 16, None, 0, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), 4, 9, 48, None, 0, _p(o), *tail), arg, "box_stats")
        refused(bs(_p(f), _p(i), 4, 3, 15, None, 0, _p(o), *tail), arg, "box_stats")          # 5K + 1 = 16 > cs
        refused(ms(None, _p(u), _p(i), None, 1, 2, 16, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), None, _p(i), None, 1, 2, 16, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), None, None, 1, 2, 16, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), _p(i), None, 1, 2, 16, None, *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), _p(i), None, -1, 2, 16, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), _p(i), None, 1, 0, 16, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), _p(i), None, 1, 2, 0, _p(o), *tail), arg, "mask_stats")
        refused(ms(_p(f), _p(u), _p(i), None, 1 << 21, 32, 16, _p(o), *tail), uns, "mask_stats")   # 2^21 * 32 * 32 = 2^31 pixels
    assert not o.any()


def test_trainer_switch_refuses_a_null_trainer_and_other_values(lib, codes):
    assert lib.rs_trainer_set_train_stats(None, 1) == codes["RS_ERR_ARG"]
    assert b"rs_trainer_set_train_stats" in lib.rs_last_error()
    assert lib.rs_trainer_set_train_stats(None, 2) == codes["RS_ERR_ARG"]


def test_the_command_line_knows_the_switch_and_defaults_it_off():
    from proj_roadsurf_amd.train_model import build_parser
    ap = build_parser()
    assert ap.parse_args(["cfg.yaml"]).train_stats is False
    assert ap.parse_args(["cfg.yaml", "--train-stats"]).train_stats is True
    import inspect
    for cls in (E.Trainer, E.MultiScaleTrainer):
        assert inspect.signature(cls.__init__).parameters["train_stats"].default is False
        assert callable(cls.set_train_stats) and callable(cls.train_stats)
