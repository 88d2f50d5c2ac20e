"""The bounds of tests/roi_cases.py held on the host: for every case, fp32 restatements of what the five RoIAlign kernels compute, in the
kernels' own operation order and from the host-compiled csrc/roi_geom.h (the driver of tests/test_roi_geom_cpu.py), lie within the bounds
tests/test_gpu_roi_bounds.py holds the kernels to, of the same float64 references.  So the references satisfy every bound and every case
reaches what it is named for without a GPU, and an edit of a bound is checked here first.

Each test prints `ROI-BOUNDS-CPU | case | form:err/bound ...`; profiles/roi_bounds/README.md is made from those lines."""
import ctypes as C

import numpy as np
import pytest

from tests import roi_cases as rc

CH = 4          # channels of the host runs (the kernels' 256 are independent of each other)


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_reaches_what_it_is_named_for(name):
    """Building a case asserts, from the host build of the header, that its RoIs take the paths the case exists for; here also that the
    levels the header assigns are oracle.assign_levels'."""
    c = rc.case(name)
    assert c.require <= c.reached
    lv, ref = rc.levels(c.rois, c.nlevels), rc.ref_levels(c)
    for slot in range(len(c.rois)):
        if slot not in c.skip_level_check:
            assert lv[slot] == ref[slot], (slot, c.rois[slot].tolist())
    print("\nROI-CASE | %s | P %d | %d entries of %d slots | %s" % (name, c.P, c.S, len(c.rois), " ; ".join(sorted(c.require))))


def test_unreachable_classes_are_unreachable():
    """The two arithmetic claims of roi_cases.UNREACHABLE, and what the searches say of the rest."""
    assert rc.MAXS % 7 and rc.MAXS % 14 and rc.MAXS % 16 == 0
    assert "P*g=511" in rc.case("capacity_p7").reached and "P*g=504" in rc.case("capacity_p14").reached and "P*g=512" in rc.case("capacity_p16").reached
    assert {"extent320_x", "extent_over_x"} <= rc.case("capacity_p14").reached
    assert 7 * rc.WMAX < rc.CELLS          # P = 7: seven tables that fit cover at most 168 cells, the window of RS_ROI_CELLS needs P = 14
    for l, sizes in ((2, rc.SIZES4[2]), (3, rc.SIZES4[3])):
        assert sizes[0] * sizes[1] < 14 * 14


def _forward_restated(c, feats, form, precision):
    """every entry through rg_pool_samples_lds (roi_align_kernel) or rg_pool_tables (roi_align_win_kernel), then the kernels' store:
    fp32 as it is, fp16 rounded, split hi + lo"""
    lib = rc.host_lib()
    lv = rc.levels(c.rois, c.nlevels)
    out = np.zeros((c.S, CH, c.P, c.P))
    for e, (kind, slot, n) in enumerate(c.entries):
        if kind != 2:
            continue
        l = int(lv[slot])
        H, W = c.sizes[l]
        F_ = np.ascontiguousarray(feats[l][0][n].astype(np.float32))
        assert np.array_equal(F_.astype(np.float64), feats[l][0][n])          # fp32(hi) + fp32(lo) is exact
        got = np.zeros((CH, c.P, c.P), np.float32)
        box = np.ascontiguousarray(c.rois[slot])
        if form == "samples":
            fast = lib.rg_pool_samples_lds(_ptr(F_), CH, H, W, _ptr(box), C.c_float(c.scales[l]), c.P, _ptr(got))
            assert fast == (0 if "slow" in c.labels[slot] else 1), (slot, fast)
            same = np.zeros_like(got)
            lib.rg_pool_samples(_ptr(F_), CH, H, W, _ptr(box), C.c_float(c.scales[l]), c.P, _ptr(same))
            assert np.array_equal(got, same), slot          # zero weights for a skipped sample == skipping it
        else:
            lib.rg_pool_tables(_ptr(F_), CH, H, W, _ptr(box), C.c_float(c.scales[l]), c.P, _ptr(got))
        if precision == "fp32":
            out[e] = got
        else:
            hi = got.astype(np.float16)
            out[e] = hi.astype(np.float64)
            if precision == "split":
                out[e] += (got - hi.astype(np.float32)).astype(np.float16).astype(np.float64)
    return out


@pytest.mark.parametrize("name", rc.FORWARD_CASES)
def test_forward_restatements_within_bound(name):
    c = rc.case(name)
    ratios = {}
    for precision in ("fp16", "fp32", "split"):
        feats = rc.features(c, CH, precision)
        ref, base = rc.forward_ref(c, [v for v, _ in feats])
        bound = rc.forward_bound(ref, base, precision)
        for form in ("samples",) if precision == "fp32" or c.P > rc.PMAX else ("tables", "samples"):
            got = _forward_restated(c, feats, form, precision)
            ratios["%s %s" % (precision, form)] = rc.ratio(got, ref, bound, "%s %s %s" % (name, precision, form))
    print("\nROI-BOUNDS-CPU | %s | %s" % (name, " ".join("%s:%.3f" % kv for kv in ratios.items())))


def _call(c, grads32, maps):
    k = rc.BwdCall()
    k.nlevels, k.n_images, k.P, k.S, k.slots_per_image, k.Cn = c.nlevels, c.n_images, c.P, c.S, c.slots_per_image, CH
    keep = [np.ascontiguousarray(c.rois), None if c.slot_list is None else np.ascontiguousarray(c.slot_list),
            None if c.n_entries is None else np.array([c.n_entries], np.int32),
            None if c.per_image_count is None else np.ascontiguousarray(c.per_image_count), np.ascontiguousarray(grads32, np.float32)]
    for l, (h, w) in enumerate(c.sizes):
        k.H[l], k.W[l], k.scale[l] = h, w, c.scales[l]
        k.d[l] = maps[l].ctypes.data
    k.rois, k.slot_list, k.n_entries, k.per_image_count, k.g = (None if a is None else a.ctypes.data for a in keep)
    return k, keep


def _backward_restated(c, grads32, pre, form, reverse):
    lib = rc.host_lib()
    lib.rg_bwd_gather32.restype = C.c_int
    maps = [p.copy() for p in pre]
    k, keep = _call(c, grads32, maps)
    n_over = None
    if form == "owner" and c.nlevels == 4:            # launch_roi_align_bwd: the owner-computes form needs four levels
        n_over = lib.rg_bwd_gather32(C.byref(k))
        lib.rg_bwd_atomic32(C.byref(k), reverse, 1)
    else:
        lib.rg_bwd_atomic32(C.byref(k), reverse, 0)
    return maps, n_over


@pytest.mark.parametrize("name", rc.BACKWARD_CASES)
def test_backward_restatements_within_bound(name):
    """The gather restatement (roi_bwd_gather_kernel's order, the RoIs it leaves to the atomic kernel added after) and the atomic restatement
    with its terms in two orders, gradients stored as half and as float, onto maps that already hold something."""
    c = rc.case(name)
    pre = rc.prefill(c, CH)
    ratios = {}
    for grad_f32 in (0, 1):
        g64, g = rc.gradients(c, CH, grad_f32)
        refs = rc.backward_ref(c, g64)
        for form in ("owner", "atomic"):
            bound = rc.backward_bound(c, refs, pre, form)
            for reverse in (0, 1):
                maps, n_over = _backward_restated(c, g.astype(np.float32), pre, form, reverse)
                if n_over is not None:
                    assert (n_over > 0) == ("bad" in c.reached), (n_over, sorted(c.reached))
                worst = 0.0
                for l in range(c.nlevels):
                    worst = max(worst, rc.ratio(maps[l], pre[l].astype(np.float64) + refs[l].grad, bound[l],
                                                "%s %s grad_f32=%d reverse=%d level %d" % (name, form, grad_f32, reverse, l)))
                ratios["%s %s%s" % (form, "float" if grad_f32 else "half", " rev" if reverse else "")] = worst
    if name == "image1_only_p7":
        assert all(not r.grad[0].any() and not r.A[0].any() for r in refs)          # the bound of image 0 is zero: its maps must keep their bits
    print("\nROI-BOUNDS-CPU | %s | %s" % (name, " ".join("%s:%.3f" % kv for kv in ratios.items())))
