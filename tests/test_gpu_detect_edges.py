"""The detection tail's index work at its edges, through the C ABI: FPN level assignment at the fp32 cut points of
detectron2's floor(4 + log2(v)), and NMS at the IoU threshold (torchvision compares the fp32 IoU with a double threshold)
in both forms of the NMS kernel (suppression mask in global memory / in LDS)."""
import ctypes as C

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import _check, load_library, make_rs_spec
from proj_roadsurf_amd.spec import EngineSpec
from tests import util as U

pytestmark = pytest.mark.gpu


def _dev(t):
    return t.contiguous().to(torch.device("cuda:0"))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ------------------------------------------------------------------ FPN level assignment
@pytest.mark.parametrize("window", [1, 0], ids=["window_kernel", "per_sample_kernel"])
@pytest.mark.parametrize("P", [7, 14])
def test_roi_align_level_assignment_at_the_cut_points(gpu_required, monkeypatch, P, window):
    """levels_out of rs_op_roi_align == detectron2's floor(4 + log2(sqrt(area)/224 + 1e-8)) in fp32 with a correctly rounded
    log2 (tests/util.py fpn_level_ref), on boxes whose v steps one float at a time across 0.5, 1 and 2 (every v a box can
    produce from 16 floats below each cut to 16 above), degenerate, very large and random boxes.  RS_ROI_WINDOW=1 runs
    roi_align_win_kernel<false>, RS_ROI_WINDOW=0 roi_align_kernel.  The sweep must reach, at each cut, a box where the
    reference and the old `v >= 2^k` rule disagree (it did on the kernels of that rule)."""
    monkeypatch.setenv("RS_ROI_WINDOW", str(window))
    lib = load_library()
    boxes = U.fpn_level_edge_boxes(seed=P)
    ref = U.fpn_level_ref(boxes)
    old = U.fpn_level_pow2_rule(boxes)
    v = U.fpn_level_v(boxes)
    for cut in U.FPN_CUTS:
        win, reach = U.fpn_level_window(cut)
        assert set(reach.tolist()) <= set(v.tolist()), f"sweep misses reachable v near {cut}"
        near = (v >= win[0]) & (v <= win[-1])
        assert bool(((ref != old) & near).any()), f"no box near {cut} where the reference and the v >= 2^k rule differ"
    n_img = 2
    rpi = (len(boxes) + n_img - 1) // n_img
    rois = np.zeros((n_img * rpi, 4), np.float32)
    rois[:len(boxes)] = boxes
    rois[len(boxes):] = [0, 0, 32, 32]
    ref_all = U.fpn_level_ref(rois)
    sizes = [(128, 128), (64, 64), (32, 32), (16, 16)]
    scales = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
    g = torch.Generator().manual_seed(3)
    fd = [_dev(torch.randn(n_img, h + 2, w + 2, 256, generator=g).half()) for h, w in sizes]
    rd = _dev(torch.from_numpy(rois))
    out = torch.empty(n_img * rpi, P, P, 256, dtype=torch.float16, device=rd.device)
    lv = torch.full((n_img * rpi,), -7, dtype=torch.int32, device=rd.device)
    vp4 = C.c_void_p * 4
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_roi_align(vp4(*[f.data_ptr() for f in fd]), (C.c_int32 * 4)(*[h for h, _ in sizes]),
                                    (C.c_int32 * 4)(*[w for _, w in sizes]), (C.c_float * 4)(*scales), 4, _ptr(rd), n_img * rpi, rpi,
                                    P, 0, _ptr(out), _ptr(lv), None), "rs_op_roi_align")
    torch.cuda.synchronize()
    got = lv.cpu().numpy().astype(np.int64)
    bad = np.nonzero(got != ref_all)[0]
    assert len(bad) == 0, [(rois[i].tolist(), float(U.fpn_level_v(rois[i:i + 1])[0]), int(got[i]), int(ref_all[i])) for i in bad[:8]]
    assert bool(torch.isfinite(out.float()).all())


# ------------------------------------------------------------------ NMS at the threshold
NMS_COUNTS = [0, 1, 63, 64, 65, 128, 1023, 1024]
NMS_INVALID = [63, 64, 127, 128, 191, 192, 1022, 1023]       # invalid entries on 64-bit mask word boundaries


def _nms_segments(t, n_seg, seed):
    """n_seg segments of capacity 1024 cycling through NMS_COUNTS; each non-trivial segment starts with the edge pairs of
    threshold t (each pair alone in its cell, the first box ahead of the second) and is filled up with dense random boxes."""
    rng = np.random.default_rng(seed)
    pairs, classes = U.nms_edge_pairs(t)
    counts = [NMS_COUNTS[s % len(NMS_COUNTS)] for s in range(n_seg)]
    boxes = np.zeros((n_seg, 1024, 4), np.float32)
    valid = np.ones((n_seg, 1024), np.uint8)
    for s, c in enumerate(counts):
        ctr = rng.uniform(0, 800, (c, 2))
        wh = rng.uniform(4, 120, (c, 2))
        b = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
        if c >= len(pairs):
            b[:len(pairs)] = pairs
        boxes[s, :c] = b
        for i in NMS_INVALID:
            if i < c:
                valid[s, i] = 0
    return boxes, valid, counts, classes


def _nms_ref(boxes, valid, counts, t):
    from oracle import maskrcnn_oracle as O
    want = np.zeros(valid.shape, bool)
    for s, c in enumerate(counts):
        v = valid[s, :c].astype(bool)
        want[s, np.nonzero(v)[0][O.nms_sorted_np(boxes[s, :c][v], t)]] = True
    return want


def _run_nms(lib, boxes, valid, counts, thresh):
    S, cap = valid.shape
    bd, cd, vd = _dev(torch.from_numpy(boxes)), _dev(torch.tensor(counts, dtype=torch.int32)), _dev(torch.from_numpy(valid))
    keep = torch.full((S, cap), 7, dtype=torch.uint8, device=bd.device)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_nms(_ptr(bd), _ptr(cd), _ptr(vd), _ptr(keep), S, cap, thresh, None), "rs_op_nms")
    torch.cuda.synchronize()
    return keep.cpu().numpy()


@pytest.mark.parametrize("segments", [8, 40], ids=["global_mask", "lds_mask"])
@pytest.mark.parametrize("t", [0.3, 0.5, 0.6, 0.7])
def test_nms_operator_at_the_threshold(gpu_required, t, segments):
    """rs_op_nms, called with the threshold the host writes into RsSpec (make_rs_spec), == the oracle's NMS (fp32 IoU >
    double threshold, torchvision's semantics) exactly, on pairs whose fp32 IoU is float32(t), the next float above and
    below, inside the kernel's +-1e-5 division band and just outside it, identical and zero-area pairs, at the 800-px
    scale; segment counts 0, 1, 63, 64, 65, 128, 1023, 1024 with invalid entries on word boundaries.  8 segments take the
    global-memory mask (two launches), 40 the LDS mask."""
    from proj_roadsurf_amd.engine import nms_thresh_f32
    lib = load_library()
    thresh = make_rs_spec(EngineSpec(nms_thresh_test=t)).nms_thresh_test
    assert thresh == nms_thresh_f32(t) == make_rs_spec(EngineSpec(rpn_nms_thresh=t)).rpn_nms_thresh
    boxes, valid, counts, classes = _nms_segments(t, segments, seed=int(t * 10) + segments)
    for cls in U.NMS_EDGE_CLASSES + ("identical", "zero_area"):
        assert cls in classes, (t, cls)
    k = _run_nms(lib, boxes, valid, counts, thresh)
    want = _nms_ref(boxes, valid, counts, t)
    for s, c in enumerate(counts):
        assert np.array_equal(k[s, :c].astype(bool), want[s, :c]), (t, segments, s, c, np.nonzero(k[s, :c].astype(bool) != want[s, :c])[0][:8])
        assert (k[s, c:] == 0).all()
    # the pairs decide on their own IoU: the second box of a pair survives exactly when its IoU is not above t
    seg = counts.index(1024)
    iou = U.nms_iou32(boxes[seg, :2 * len(classes):2], boxes[seg, 1:2 * len(classes):2])[0]
    assert np.array_equal(k[seg, 1:2 * len(classes):2].astype(bool), ~(iou.astype(np.float64) > t))


@pytest.mark.parametrize("segments", [1, 40])
def test_nms_operator_torchvision_kat_at_0_6(gpu_required, segments):
    """[0,0,100,100] then [0,0,100,60]: fp32 IoU = float32(0.6) = 0.6000000238 > 0.6, so torchvision suppresses the second box
    at threshold 0.6 (and at 0.5), and keeps it at 0.7.  Through the threshold make_rs_spec writes, in both NMS forms."""
    lib = load_library()
    boxes = np.zeros((segments, 1024, 4), np.float32)
    boxes[:, 0] = [0, 0, 100, 100]
    boxes[:, 1] = [0, 0, 100, 60]
    valid = np.ones((segments, 1024), np.uint8)
    counts = [2] * segments
    for t, second in ((0.6, 0), (0.5, 0), (0.7, 1)):
        k = _run_nms(lib, boxes, valid, counts, make_rs_spec(EngineSpec(nms_thresh_test=t)).nms_thresh_test)
        assert (k[:, 0] == 1).all() and (k[:, 1] == second).all(), (t, k[:, :2])
