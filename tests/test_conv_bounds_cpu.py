"""The per-element bound of tests/conv_cases.py without a GPU: an emulation of a correct fp16 kernel (fp32 accumulation of the stored operands,
one rounding) passes it, four seeded kernel faults fail it, and three of those pass what the operator tests asserted before (one global
tolerance of 2e-3 of the largest output, and equal absolute sums with and without the halo of a zero-filled buffer) -- the gap this closes."""
import numpy as np
import pytest

from tests import conv_cases as cc


def _case(tag):
    return next(c for c in cc.bound_cases() if c.tag == tag)


EMULATED = ["fp16 conv3x3 s1 256->256 2x24x20 res up relu", "fp16 conv1x1 s1 256->1024 2x24x20 res relu", "fp16 conv1x1 s1 64->64 1x13x11 res relu"]


@pytest.fixture(scope="module", params=EMULATED)
def problem(request):
    P = cc.build(_case(request.param))
    return P, cc.emulate(P)


def _old_criterion(P, buf):
    """tests/test_gpu_conv.py before: the buffer starts as zeros, so what the sentinel marks as never written reads as zero"""
    o = np.where(buf == cc.SENTINEL, 0, buf).astype(np.float32)
    inner = cc.interior(P, o)
    if float(np.abs(o).sum()) != pytest.approx(float(np.abs(inner).sum()), rel=1e-6):
        return False
    ref = P.ref.astype(np.float32)
    return float(np.abs(inner - ref).max()) <= 2e-3 * max(1.0, float(np.abs(ref).max()))


def _rejected(P, buf):
    try:
        cc.check_output(P, buf)
    except AssertionError:
        return True
    return False


def test_emulated_kernel_is_inside_the_bound(problem):
    P, buf = problem
    worst = cc.check_output(P, buf)
    print(f"    {P.case.tag}: largest err / bound {worst:.3f}")
    assert 0.5 < worst <= 1.0           # the rounding term is attained, not merely respected
    assert _old_criterion(P, buf)


def test_a_missing_k_slice_is_rejected(problem):
    """the input channel of smallest magnitude zeroed: a K slice the kernel never multiplied"""
    P, _ = problem
    x = P.x.copy()
    mag = np.abs(x.astype(np.float64)).sum((0, 1, 2))
    x[..., int(np.argmin(mag))] = 0
    buf = cc.emulate(P, x=x)
    assert _rejected(P, buf)
    assert _old_criterion(P, buf), "the global tolerance saw the missing slice too"


def _pixel(P, buf, m):
    """the channels of pixel m (row-major over n, y, x) of a buffer: a view"""
    n, r = divmod(int(m), P.oh * P.ow)
    return buf[n, P.out_halo + r // P.ow, P.out_halo + r % P.ow]


def _ragged_tail(P):
    """first pixel (row-major over n, y, x) past the last full 128-pixel tile"""
    m = P.case.n * P.oh * P.ow
    assert m % 128 != 0
    return m // 128 * 128


def test_an_unwritten_pixel_of_the_ragged_tail_is_rejected(problem):
    """One pixel row of the last, partial tile left as it was: all its channels, and (the store a lane can miss: 16 bytes) the eight
    consecutive channels of the tail whose outputs are smallest.  The whole row moves channels by far more than 2e-3 of the largest output, so
    the old criterion sees it as well; the eight channels where ReLU left (near) zeros it does not -- a zero-filled buffer already held them."""
    P, clean = problem
    cout = P.ref.shape[3]
    tail = np.arange(_ragged_tail(P), P.case.n * P.oh * P.ow)
    buf = clean.copy()
    _pixel(P, buf, tail[-1])[:] = cc.SENTINEL
    assert _rejected(P, buf)
    groups = np.abs(P.ref.reshape(-1, cout)[tail]).reshape(len(tail), cout // 8, 8).max(-1)
    pix, grp = np.unravel_index(int(np.argmin(groups)), groups.shape)
    buf = clean.copy()
    _pixel(P, buf, tail[pix])[8 * grp:8 * grp + 8] = cc.SENTINEL
    assert _rejected(P, buf)
    assert _old_criterion(P, buf), "the global tolerance saw the unwritten store too"


def test_a_zero_written_into_the_halo_is_rejected(problem):
    P, clean = problem
    buf = clean.copy()
    buf[0, 0, 3, 5] = 0
    assert _rejected(P, buf)
    assert _old_criterion(P, buf), "the sum over the halo saw a zero"


def test_two_swapped_channels_are_rejected(problem):
    """at the pixel and the channel pair whose outputs differ by the largest multiple of the sum of their bounds (more than that sum, asserted)"""
    P, clean = problem
    cout = P.ref.shape[3]
    ref, bnd = P.ref.reshape(-1, cout), P.bound.reshape(-1, cout)
    a, b = np.argmin(ref / bnd, 1), np.argmax(ref / bnd, 1)
    rows = np.arange(len(ref))
    margin = np.abs(ref[rows, a] - ref[rows, b]) / (bnd[rows, a] + bnd[rows, b])
    m = int(np.argmax(margin))
    assert margin[m] > 1.0
    buf = clean.copy()
    px = _pixel(P, buf, m)
    px[a[m]], px[b[m]] = px[b[m]].copy(), px[a[m]].copy()
    assert _rejected(P, buf)


def test_engine_layer_classes_are_derived_and_reach_what_the_grid_lacked():
    classes = cc.engine_classes()
    assert classes
    assert any(c[:4] == (128, 3, 1, 128) for c in classes)                       # a 3x3 with 128 channels
    assert any(c[:4] == (512, 3, 1, 512) for c in classes)                       # ... with 512
    assert any(c[0] == 12544 and c[1] == 1 for c in classes)                     # the FC
    assert any(c[1] == 1 and c[6] == 15 for c in classes)                        # a variant-15 1x1
    assert not any(c[6] in (13, 21) for c in classes)
    cases = cc.bound_cases()
    tags = [c.tag for c in cases]
    assert len(set(tags)) == len(tags)
    for c in cases:
        assert -1 in c.required and set(c.required) <= set(c.variants)
        assert not any((c.tag, v) in cc.EXPECTED_REFUSED for v in c.required), c.tag
    fc = [c for c in cases if c.cin == 12544]
    assert [(c.n, c.h, c.w) for c in fc] == [(1, cc.FC_M, 1)] and set(fc[0].variants) == {-1, 7, 12}


def test_every_reference_keeps_clear_of_the_clamp_and_of_the_sentinel():
    """build() asserts it per case (|ref| < 60000; an element that keeps the sentinel is outside its bound): here for the deepest and the widest"""
    for tag in ("fp16 class conv1x1 s1 12544->1024 relu 1x143x1", "split conv3x3 s1 256->1024 2x24x20 relu", "dgrad 1x1 s2 256<-1024 2x24x20 mask"):
        P = cc.build(_case(tag))
        assert P.written.any() and np.all(P.bound[P.written] > 0)


def test_every_tail_reference_keeps_its_flagged_share_small():
    """build_bneck() asserts it: fewer than 5 % (10 % on zero-mean conv2 weights, conv_cases.build_bneck) of t2 within their accumulation noise of an fp16 rounding boundary, so that the step those may come out
    off by widens the bound of few elements of `out`; and the split tails flag none (nothing is rounded in between)"""
    tails = [c for c in cc.bound_cases() if c.op == "bneck"]
    assert len(tails) == 26 and sum(c.w2_mean == 0.0 for c in tails) == 2        # the grid's 24 and the two fp16 tails on zero-mean conv2 weights
    for c in tails:
        P = cc.build_bneck(c)
        assert (P.flagged == 0.0) if c.split else (0.0 < P.flagged < c.flag_limit)
        assert c.flag_limit == (0.10 if c.w2_mean == 0.0 else 0.05)
        assert np.all(P.out_bound > 0) and np.all(P.t1n_bound > 0)
