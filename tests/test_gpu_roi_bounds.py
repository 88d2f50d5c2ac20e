"""Every form of the five RoIAlign kernels against float64, element by element, over the cases of tests/roi_cases.py (found by search with
the host build of csrc/roi_geom.h; tests/test_roi_bounds_cpu.py holds the same bounds on fp32 restatements).  Forward: fp16 windowed, fp16
per-sample, fp32 per-sample, split windowed, split per-sample, against oracle.maskrcnn_oracle.roi_align_one on float64 maps.  Backward:
owner-computes and atomic, gradients stored as half and as float, against float64 autograd through oracle.train_oracle.roi_align_diff.

The buffers a kernel writes start as the bit pattern of 30000.0 (halo of the pooled output, entries past the device count, halo of the
gradient maps) or as N(0,1) values (interior of the gradient maps: the backward accumulates); the halos of the buffers it reads hold
30000.0 too.  After a run every element is either still that pattern, bit for bit, or inside its bound -- none is left out.

Each test prints `ROI-BOUNDS | case | form:err/bound ...`; profiles/roi_bounds/README.md is made from those lines."""
import ctypes as C
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import _check, load_library
from tests import roi_cases as rc

pytestmark = pytest.mark.gpu

CH = 256
FORWARD_FORMS = [("fp16 windowed", "fp16", "1"), ("fp16 per-sample", "fp16", "0"), ("fp32 per-sample", "fp32", "1"), ("split windowed", "split", "1"),
                 ("split per-sample", "split", "2")]                      # name, precision, RS_ROI_WINDOW
BACKWARD_FORMS = [("owner", "0"), ("atomic", "1")]                        # name, RS_ROI_BWD_ATOMIC
LEVEL_UNSET = -7


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _nhwc_halo(planes, pad, fill):
    """planes: arrays [n][C][H][W] -> [len(planes)][n][H+2p][W+2p][C], the halo holding `fill`"""
    n, ch, h, w = planes[0].shape
    out = np.full((len(planes), n, h + 2 * pad, w + 2 * pad, ch), fill, planes[0].dtype)
    for k, p in enumerate(planes):
        out[k, :, pad:pad + h, pad:pad + w] = p.transpose(0, 2, 3, 1)
    return out


def _arrays(c):
    """heights, widths, scales as the ABI's arrays of four, and the entry plumbing on the device"""
    pad4 = lambda v, ty: (ty * 4)(*(list(v) + [0] * (4 - len(v))))
    hs, ws = pad4([h for h, _ in c.sizes], C.c_int32), pad4([w for _, w in c.sizes], C.c_int32)
    sc = pad4(c.scales, C.c_float)
    dev = SimpleNamespace(rois=_dev(c.rois), slot_list=_dev(c.slot_list), n_entries=_dev(None if c.n_entries is None else np.array([c.n_entries], np.int32)),
                           per_image_count=_dev(c.per_image_count), order=_dev(c.order))
    return hs, ws, sc, dev


def _untouched(a, what):
    want = np.full(1, rc.SENTINEL, a.dtype)
    assert a.tobytes() == np.broadcast_to(want, a.shape).tobytes(), what


def _run_forward(lib, c, planes_dev, precision, arrays):
    hs, ws, sc, dev = arrays
    PP = c.P + 2 * c.out_halo
    np_dt = np.float32 if precision == "fp32" else np.float16
    n_planes = 2 if precision == "split" else 1
    out = _dev(np.full((n_planes, c.S, PP, PP, CH), rc.SENTINEL, np_dt))
    lv = _dev(np.full(c.S, LEVEL_UNSET, np.int32))
    vp4 = C.c_void_p * 4
    feats = vp4(*([t[0].data_ptr() for t in planes_dev] + [None] * (4 - c.nlevels)))
    lo = (C.c_int64 * 4)(*([t[0].numel() for t in planes_dev] + [0] * (4 - c.nlevels)))
    rc_ = lib.rs_op_roi_align_form(feats, lo, hs, ws, sc, c.nlevels, _p(dev.rois), c.S, c.slots_per_image, c.P, c.out_halo,
                                   {"fp16": 0, "fp32": 1, "split": 2}[precision], _p(out), C.c_int64(out[0].numel()), _p(dev.slot_list), _p(dev.n_entries),
                                   _p(dev.per_image_count), _p(dev.order), _p(lv), None)
    _check(lib, rc_, "rs_op_roi_align_form")
    torch.cuda.synchronize()
    return out.cpu().numpy(), lv.cpu().numpy()


def _check_forward(c, buf, lv, ref, bound, what):
    """buf [planes][S][PP][PP][CH]: the halo and the entries past the count keep their bits; empty slots are zeros in every plane; the rest
    is within its bound; the levels are oracle.assign_levels'."""
    h, P = c.out_halo, c.P
    inner = buf[:, :, h:h + P, h:h + P]
    if h:
        edge = buf.copy()
        edge[:, :, h:h + P, h:h + P] = rc.SENTINEL
        _untouched(edge, what + ": the halo of the pooled output was written")
    want_lv = rc.ref_levels(c)
    value = np.zeros((c.S, CH, P, P))
    for e, (kind, slot, n) in enumerate(c.entries):
        if kind == 0:
            _untouched(inner[:, e], "%s: entry %d lies past the device count and was written" % (what, e))
            assert lv[e] == LEVEL_UNSET
            value[e] = ref[e]                       # compared above, bit for bit; nothing more to hold it to
            continue
        if kind == 1:
            assert not inner[:, e].any(), "%s: empty slot, entry %d: every plane must be zero" % (what, e)
            assert lv[e] == LEVEL_UNSET
        else:
            assert lv[e] == (0 if slot in c.skip_level_check else want_lv[slot]), (what, e, slot, int(lv[e]), int(want_lv[slot]))
        value[e] = inner[:, e].astype(np.float64).sum(0).transpose(2, 0, 1)
    return rc.ratio(value, ref, bound, what)


@pytest.mark.parametrize("name", rc.FORWARD_CASES)
def test_forward_forms_within_bound_of_float64(gpu_required, monkeypatch, name):
    lib = load_library()
    c = rc.case(name)
    arrays = _arrays(c)
    t0 = time.time()
    ratios, problems = {}, {}
    for form, precision, window in FORWARD_FORMS:
        if precision not in problems:
            feats = rc.features(c, CH, precision)
            ref, base = rc.forward_ref(c, [v for v, _ in feats])
            problems[precision] = ([_dev(_nhwc_halo(planes, 1, rc.SENTINEL)) for _, planes in feats], ref, rc.forward_bound(ref, base, precision))
        planes_dev, ref, bound = problems[precision]
        monkeypatch.setenv("RS_ROI_WINDOW", window)
        buf, lv = _run_forward(lib, c, planes_dev, precision, arrays)
        ratios[form] = _check_forward(c, buf, lv, ref, bound, "%s %s" % (name, form))
    print("\nROI-BOUNDS | %s | %s | %.1f s" % (name, " ".join("%s:%.3f" % kv for kv in ratios.items()), time.time() - t0))


def _run_backward(lib, c, maps0, dout, grad_f32, arrays):
    hs, ws, sc, dev = arrays
    maps = [_dev(m) for m in maps0]
    vp4 = C.c_void_p * 4
    d4 = vp4(*([m.data_ptr() for m in maps] + [None] * (4 - c.nlevels)))
    rc_ = lib.rs_op_roi_align_bwd_form(d4, hs, ws, sc, c.nlevels, _p(dev.rois), c.S, c.slots_per_image, c.n_images, c.P, c.out_halo, grad_f32, _p(dout),
                                       _p(dev.slot_list), _p(dev.n_entries), _p(dev.per_image_count), None)
    _check(lib, rc_, "rs_op_roi_align_bwd_form")
    torch.cuda.synchronize()
    return [m.cpu().numpy() for m in maps]


@pytest.mark.parametrize("name", rc.BACKWARD_CASES)
def test_backward_forms_within_bound_of_float64(gpu_required, monkeypatch, name):
    lib = load_library()
    c = rc.case(name)
    arrays = _arrays(c)
    t0 = time.time()
    pre = rc.prefill(c, CH)
    maps0 = [_nhwc_halo((p,), 1, rc.SENTINEL)[0] for p in pre]
    ratios = {}
    for grad_f32 in (0, 1):
        g64, g = rc.gradients(c, CH, grad_f32)
        refs = rc.backward_ref(c, g64)
        # [S][PP][PP][CH], the halo of every entry's gradient tile holding 30000: the kernels read the interior only
        dout = _dev(_nhwc_halo((g,), c.out_halo, rc.SENTINEL)[0])
        for form, atomic in BACKWARD_FORMS:
            monkeypatch.setenv("RS_ROI_BWD_ATOMIC", atomic)
            bound = rc.backward_bound(c, refs, pre, form)
            got = _run_backward(lib, c, maps0, dout, grad_f32, arrays)
            what = "%s %s %s" % (name, form, "float" if grad_f32 else "half")
            worst = 0.0
            for l, (m, m0) in enumerate(zip(got, maps0)):
                edge = m.copy()
                edge[:, 1:-1, 1:-1] = rc.SENTINEL
                _untouched(edge, "%s: the halo of gradient map %d was written" % (what, l))
                worst = max(worst, rc.ratio(m[:, 1:-1, 1:-1].transpose(0, 3, 1, 2), pre[l].astype(np.float64) + refs[l].grad, bound[l], "%s level %d" % (what, l)))
            ratios["%s %s" % (form, "float" if grad_f32 else "half")] = worst
            if form == "owner" and c.nlevels == 4 and "bad" not in c.reached:          # no atomics in the call: the same bits on every run
                again = _run_backward(lib, c, maps0, dout, grad_f32, arrays)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), what + ": two runs of the owner-computes form differ"
    print("\nROI-BOUNDS | %s | %s | %.1f s" % (name, " ".join("%s:%.3f" % kv for kv in ratios.items()), time.time() - t0))
