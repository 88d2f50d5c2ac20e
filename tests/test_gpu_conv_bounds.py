"""Every tile variant of every convolution operator against float64, element by element (tests/conv_cases.py: the case grid of
tools/parity/conv_op_compare.py plus the layer classes the engine's tile table launches; the reference on exactly the operands the GPU
received; the bound).  The output buffers start as the bit pattern of 30000.0: after a run the halo, and every pixel the kernel does not own,
still hold it bit for bit, and every other element is inside its bound, which an unwritten 30000 is not.  A variant the library refuses fails
unless conv_cases.EXPECTED_REFUSED lists it with the check that justifies it.  Bit identity across variants is asserted where DESIGN.md
claims it: all split variants (3.1d), and the register-weight kernels 22 / 23 / 25 / 26 against the 128 x 256 tile.

Each test prints `BOUNDS | case | variant:err/bound ... | distinct outputs`; profiles/conv_bounds/README.md is made from those lines."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from proj_roadsurf_amd.engine import load_library
from tests import conv_cases as cc

pytestmark = pytest.mark.gpu

CASES = cc.bound_cases()
CONV_CASES = [c for c in CASES if c.op != "bneck"]
BNECK_CASES = [c for c in CASES if c.op == "bneck"]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lo(t):
    return C.c_int64(0 if t is None else t[0].numel())


class _Operands:
    """the operands of a problem on the device, uploaded once for all variants"""

    def __init__(self, P, names):
        for name in names:
            setattr(self, name, _dev(getattr(P, name, None)))


def _run_conv(lib, P, D, variant):
    c = P.case
    od = _dev(cc.empty_output(P))
    pad = P.pad
    if c.op == "dgrad":
        rc = lib.rs_op_conv2d_dgrad(_p(D.x), _p(D.w), _p(od), _p(D.res), _p(D.res32), _p(D.mask), _p(D.down), c.n, c.h, c.w, c.cin, P.ho, P.wo, c.cout,
                                    c.k, c.k, c.stride, c.k // 2, P.K, 1, variant, None)
    elif c.op == "dual":
        rc = lib.rs_op_conv2d_dual(_p(D.x), _p(D.x2), _p(D.w), _p(D.bias), _p(od), c.n, c.h, c.w, c.cin, P.in_halo, 1, 1, 1, 0,
                                   c.h * c.stride2, c.w * c.stride2, c.cin2, 1, c.stride2, c.cout, P.K, 1, int(c.relu), variant, None)
    elif c.split:
        rows = c.cout * (4 if c.deconv else 1)
        rc = lib.rs_op_conv2d_split(_p(D.x), _lo(D.x), _p(D.w), C.c_int64(rows * P.K), _p(D.wscale), _p(D.bias), _p(od), C.c_int64(0) if c.out_f32 else _lo(od),
                                    _p(D.res), _lo(D.res), _p(D.up), _lo(D.up), c.n, c.h, c.w, c.cin, P.in_halo, c.k, c.k, c.stride, pad, c.cout, P.K, P.out_halo,
                                    int(c.relu), int(c.out_f32), int(c.deconv), variant, None)
    else:
        rc = lib.rs_op_conv2d(_p(D.x), _p(D.w), _p(D.bias), _p(od), _p(D.res), _p(D.up), c.n, c.h, c.w, c.cin, P.in_halo, c.k, c.k, c.stride, pad, c.cout, P.K,
                              P.out_halo, int(c.relu), int(c.out_f32), int(c.deconv), variant, 1, None)
    torch.cuda.synchronize()
    return rc, od.cpu().numpy()


def _refusal_is_expected(lib, case, variant):
    want = cc.EXPECTED_REFUSED.get((case.tag, variant))
    msg = lib.rs_last_error().decode(errors="replace")
    assert want is not None and variant not in case.required, f"{case.tag}: variant {variant} refused: {msg}"
    assert want in msg, f"{case.tag}: variant {variant} refused with '{msg}', the table expects '{want}'"


@pytest.mark.parametrize("case", CONV_CASES, ids=[c.tag for c in CONV_CASES])
def test_conv_variants_within_bound_of_float64(gpu_required, case):
    lib = load_library()
    P = cc.build(case)
    D = _Operands(P, ("x", "x2", "w", "wscale", "bias", "res", "up", "res32", "mask", "down"))
    ratios, bits, refused = {}, {}, []
    for v in case.variants:
        rc, buf = _run_conv(lib, P, D, v)
        if rc != 0:
            _refusal_is_expected(lib, case, v)
            refused.append(v)
            continue
        ratios[v] = cc.check_output(P, buf)
        bits[v] = hashlib.sha256(buf.tobytes()).hexdigest()
    print("\nBOUNDS | %s | %s | %d distinct%s" % (case.tag, " ".join("%d:%.3f" % kv for kv in ratios.items()), len(set(bits.values())),
                                                 " | refused %s" % refused if refused else ""))
    if case.split:
        assert len(set(bits.values())) == 1, f"split variants differ in bits: {sorted(bits.items(), key=lambda kv: kv[1])}"
    for v in cc.WREG:
        if v in bits and 14 in bits:
            assert bits[v] == bits[14], f"variant {v} differs in bits from the 128x256 tile"


def _run_bneck(lib, P, D):
    c = P.case
    shape = lambda ch: ((2,) if c.split else ()) + (c.n, c.h + 2, c.w + 2, ch)
    out, t1n = (_dev(np.full(shape(ch), cc.SENTINEL, np.float16)) for ch in (4 * c.width, c.width))
    nx = lambda t: _p(t) if c.nxt else None
    if c.split:
        rc = lib.rs_op_bneck_tail_split(_p(D.t1), _lo(D.t1), _p(D.w2), _p(D.s2), _p(D.b2), _p(D.w3), _p(D.s3), _p(D.b3), None if c.proj else _p(D.x), _lo(D.x),
                                        _p(out), _lo(out), nx(D.w1), nx(D.s1), nx(D.b1), nx(t1n), _lo(t1n), _p(D.x) if c.proj else None, _lo(D.x),
                                        c.n, c.h, c.w, c.width, None)
    else:
        rc = lib.rs_op_bneck_tail(_p(D.t1), _p(D.w2), _p(D.b2), _p(D.w3), _p(D.b3), None if c.proj else _p(D.x), _p(out), nx(D.w1), nx(D.b1), nx(t1n),
                                  _p(D.x) if c.proj else None, _p(D.wsc) if c.proj else None, c.n, c.h, c.w, c.width, None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), t1n.cpu().numpy()


@pytest.mark.parametrize("case", BNECK_CASES, ids=[c.tag for c in BNECK_CASES])
def test_bneck_tail_within_bound_of_float64(gpu_required, case):
    lib = load_library()
    P = cc.build_bneck(case)
    D = _Operands(P, ("t1", "x", "w2", "s2", "b2", "w3", "s3", "b3", "w1", "s1", "b1", "wsc"))
    rc, out, t1n = _run_bneck(lib, P, D)
    assert rc == 0, f"{case.tag}: refused: {lib.rs_last_error().decode(errors='replace')}"
    r_out = cc.check_map(case.tag + " out", out, P.out_ref, P.out_bound, P.planes)
    if case.nxt:
        r_t1n = cc.check_map(case.tag + " t1n", t1n, P.t1n_ref, P.t1n_bound, P.planes)
    else:
        r_t1n = 0.0
        cc.assert_all_untouched(t1n, "t1n written without a next conv1")
    print("\nBOUNDS | %s | out:%.3f t1n:%.3f | %.2f %% of t2 within its noise of a rounding boundary" % (case.tag, r_out, r_t1n, 100 * P.flagged))


# One case per depth for the fp32-MFMA mode (use_glds = -1, csrc/ref_f32.hip) on the fp16-representable operands of the fp16 case: its largest
# err / s is what conv_cases.F32_MODE_ERR records, and the allowance of the fp16 kernels covers 1.5 times it.
F32_MODE_CASES = {64: "fp16 conv1x1 s1 64->256 2x24x20 res relu", 256: "fp16 conv1x1 s1 256->256 2x24x20 res relu", 576: "fp16 conv3x3 s1 64->256 2x24x20 relu",
                  2304: "fp16 conv3x3 s1 256->256 2x24x20 relu", 4608: "fp16 class conv3x3 s1 512->512 relu 2x24x20",
                  12544: "fp16 class conv1x1 s1 12544->1024 relu 1x143x1"}


@pytest.mark.parametrize("k", sorted(F32_MODE_CASES))
def test_fp32_mode_noise_is_inside_the_allowance(gpu_required, k):
    lib = load_library()
    case = next(c for c in CASES if c.tag == F32_MODE_CASES[k])
    P = cc.build(case)
    assert P.K == k
    f32 = lambda a: None if a is None else _dev(a.astype(np.float32))
    x, w, bias, res = f32(P.x), f32(P.w), _dev(P.bias), f32(P.res)
    od = _dev(np.full((case.n, P.oh + 2 * P.out_halo, P.ow + 2 * P.out_halo, case.cout), cc.SENTINEL, np.float32))
    rc = lib.rs_op_conv2d(_p(x), _p(w), _p(bias), _p(od), _p(res), None, case.n, case.h, case.w, case.cin, P.in_halo, case.k, case.k, case.stride, P.pad,
                          case.cout, P.K, P.out_halo, int(case.relu), 1, 0, -1, -1, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.rs_last_error()
    buf = od.cpu().numpy()
    e = float((np.abs(cc.interior(P, buf).astype(np.float64) - P.ref) / P.s).max())
    print("\nF32MODE | K %d | %s | err / s %.3e | A(K) %.3e | allowance %.3e" % (k, case.tag, e, cc.A(k), cc.allowance(k)))
    if P.out_halo:
        cc.assert_halo_untouched(buf, P.out_halo, "the fp32 kernel wrote into the halo")
    assert 1.5 * e <= cc.allowance(k), "the allowance of the fp16 kernels does not cover 1.5 x the fp32 mode's noise at this depth"
