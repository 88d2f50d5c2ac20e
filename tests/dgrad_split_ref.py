"""The arithmetic of the fp32 trainer's input gradient on split operands (csrc/conv_wgrad.hip: the abs-max and plane passes and
split_rows_kernel; csrc/conv_igemm.hip: the TRAIN && SPLIT instantiation; csrc/conv_tile.h: epi_values_dgrad_split) stated in numpy, its
error bound, and the inputs its tests share.

  dY:   e_dy   = 14 - floor(log2 amax) over the tensor (0 for an all-zero or a non-finite one)        [wgrad_split_ref.exponent]
        hi, lo = fp16(dy 2^e_dy), fp16(dy 2^e_dy - hi)                                               [wgrad_split_ref.planes]
  W^T:  e(row) = 13 - floor(log2 max|row|) clipped to +-100 (0 for a zero row); hi, lo of w 2^e(row); inv(row) = 2^-e(row)
  dX    = (W_hi . dY_lo + W_hi . dY_hi + W_lo . dY_hi) * inv(row) * 2^-e_dy                          lo . lo dropped
  then  + res + the 2x2 sum of down + res32 in fp32, in that order, then the mask (saved activation > 0)

Products of two fp16 values are exact in the matrix cores' fp32 accumulator; here they are accumulated in float64, so the statement
carries the representation error alone and the kernel adds the accumulation-order error of its fp32 sums.

Bound per element of the GEMM, T = KH KW Cout_pad terms:

  |dx - exact| <= 2^-20 S + 2^-36 T max|dy| rowmax|w| + E_f32,       S = sum |dy| |w| over the element's terms

  * operands in the normal fp16 range after scaling keep 22 significand bits each, and lo . lo (<= 2^-22 of the product) is dropped:
    3 * 2^-22 < 2^-20 of S;
  * a dY element below 2^-18 of the tensor maximum leaves the normal range of its lo half: its hi + lo is off by at most 2^-25 in scaled
    units, 2^-39 of the tensor maximum (the scaled maximum is >= 2^14).  A weight below 2^-17 of its row maximum likewise: at most 2^-25
    scaled, 2^-38 of the row maximum (scaled >= 2^13).  Per term <= 2^-39 max|dy| |w| + 2^-38 |dy| rowmax|w| <= 3 * 2^-39 max|dy| rowmax|w|;
    the bound takes 2^-36, the weight gradient's constant;
  * E_f32 is measured by the GPU tests from the fp32 matrix-core kernel on the same operands (rs_op_conv2d, use_glds = -1).
With addends the at most six fp32 additions of the epilogue allow 6 * 2^-24 (|gemm| + sum |addend|) more (epilogue_allowance)."""
import numpy as np

from tests.wgrad_split_ref import FAMILIES, exponent, planes      # noqa: F401  (the dY side is the weight gradient's, re-exported)
from tests import wgrad_split_ref as _W


def row_planes(w: np.ndarray):
    """w [rows][k] fp32 -> (hi [rows][k] fp16, lo [rows][k] fp16, inv [rows] fp32, e [rows] int)."""
    w = np.ascontiguousarray(w, np.float32)
    mx = np.abs(w).max(axis=1)
    _, ex = np.frexp(mx.astype(np.float64))                # mx = m 2^ex, m in [0.5, 1): floor(log2 mx) = ex - 1, subnormals included
    e = np.where((mx > 0) & np.isfinite(mx), 13 - (ex - 1), 0)
    e = np.clip(e, -100, 100).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.ldexp(w.astype(np.float64), e[:, None]).astype(np.float32)          # exact unless the clip lets it leave the range
        hi = t.astype(np.float16)
        lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, np.ldexp(np.float32(1), -e).astype(np.float32), e


def dgrad_split(dy: np.ndarray, w: np.ndarray) -> np.ndarray:
    """dy [M][T], w [rows][T] fp32 (T = the GEMM's K: taps x padded Cout) -> dX [M][rows] float64 by the kernel's representation."""
    e_dy = exponent(dy)
    yh, yl = (p.astype(np.float64) for p in planes(dy, e_dy))
    wh, wl, inv, _ = row_planes(w)
    wh, wl = wh.astype(np.float64), wl.astype(np.float64)
    acc = yl @ wh.T
    acc += yh @ wh.T
    acc += yh @ wl.T
    return np.ldexp(acc * inv.astype(np.float64)[None, :], -e_dy)


def bound(S: np.ndarray, t_terms: int, dy_max: float, w_rowmax: np.ndarray) -> np.ndarray:
    """The two derived terms for S [M][rows] and w_rowmax [rows]; the GPU tests add the fp32 kernel's measured E_f32."""
    return 2.0 ** -20 * np.asarray(S, np.float64) + 2.0 ** -36 * t_terms * float(dy_max) * np.asarray(w_rowmax, np.float64)[None, :]


def epilogue_allowance(gemm: np.ndarray, addends_abs_sum: np.ndarray) -> np.ndarray:
    return 6.0 * 2.0 ** -24 * (np.abs(gemm) + addends_abs_sum)


def family(name: str, rng: np.random.Generator, dy_shape, w_shape):
    """(dy, w): dY of wgrad_split_ref.family against ordinary weights -- gaussian rows of 0.05 whose magnitudes differ row by row
    (0.1 .. 10), which is what the per-row scale is for."""
    dy, _ = _W.family(name, rng, dy_shape, (1, 1))
    w = (rng.standard_normal(w_shape) * 0.05).astype(np.float32)
    w *= np.exp2(rng.uniform(-3.3, 3.3, (w_shape[0],) + (1,) * (len(w_shape) - 1))).astype(np.float32)
    return dy, w
