"""The arithmetic of the split-operand weight gradient (csrc/conv_wgrad.hip: wgrad_split_amax_kernel, wgrad_split_planes_kernel,
conv_wgrad_split_kernel) stated in numpy, its error bound, and the input families its tests share.

  e       = 14 - floor(log2(amax)) per operand tensor (amax over the finite values; 0 for an all-zero or a non-finite tensor)
  t       = v * 2^e                       exact, |t| < 2^15
  hi, lo  = fp16(t), fp16(t - hi)         round to nearest even
  dW      = (dY_hi^T X_lo + dY_hi^T X_hi + dY_lo^T X_hi) * 2^-(e_dy + e_x)        lo . lo dropped

The products of two fp16 values are exact in the matrix cores' fp32 accumulator; here they are accumulated in float64, so this statement
carries the representation error alone (the kernel adds the accumulation-order error of its fp32 sums).

Bound per element, M terms:  |dW - exact| <= 2^-20 S + 2^-36 M max|dy| max|x|,   S = sum |dy| |x| over the element's terms.
  * an element in the normal fp16 range after scaling: |t - hi - lo| <= 2^-22 |t|; two operands and the dropped lo . lo product give
    3 * 2^-22 < 2^-20 of S;
  * below that range the absolute error of hi + lo is <= 2^-25 in scaled units, at most 2^-39 of the tensor's maximum (the scaled
    maximum is >= 2^14); per term that is <= 2^-39 max|dy| |x| + 2^-39 |dy| max|x| <= 2^-38 max|dy| max|x|, and the bound takes 2^-36."""
import numpy as np


def exponent(a: np.ndarray) -> int:
    a = np.asarray(a, np.float32)
    if not np.isfinite(a).all():
        return 0
    amax = float(np.abs(a).max()) if a.size else 0.0
    if amax == 0.0:
        return 0
    _, ex = np.frexp(amax)          # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    return 14 - (int(ex) - 1)


def planes(a: np.ndarray, e: int):
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.ldexp(np.asarray(a, np.float32), e).astype(np.float32)
        hi = t.astype(np.float16)
        lo = (t - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def wgrad_split(dy: np.ndarray, x: np.ndarray) -> np.ndarray:
    """dy [M][Cout], x [M][K] fp32 -> dW [Cout][K] float64 by the kernel's representation."""
    e_dy, e_x = exponent(dy), exponent(x)
    yh, yl = (p.astype(np.float64) for p in planes(dy, e_dy))
    xh, xl = (p.astype(np.float64) for p in planes(x, e_x))
    acc = yh.T @ xl
    acc += yh.T @ xh
    acc += yl.T @ xh
    return np.ldexp(acc, -(e_dy + e_x))


def bound(S: np.ndarray, m_terms: int, dy_max: float, x_max: float) -> np.ndarray:
    """The two derived terms; the GPU tests add the fp32 kernel's measured accumulation-order error."""
    return 2.0 ** -20 * np.asarray(S, np.float64) + 2.0 ** -36 * m_terms * float(dy_max) * float(x_max)


FAMILIES = ("gaussian", "heavy_tail", "small_times_large")


def family(name: str, rng: np.random.Generator, dy_shape, x_shape):
    """fp32 (dy, x) of the given shapes.  gaussian: the operator tests' inputs.  heavy_tail: dY magnitudes 2^-35 .. 2^-20 of two planted
    entries near 1 (most of the tensor is subnormal in the hi plane) against a ReLU'd X.  small_times_large: gradients of 1e-7 without a
    loss scale against activations of 3e3 -- the lo planes of both would be lost without the per-tensor scale."""
    dy = rng.standard_normal(dy_shape).astype(np.float32)
    x = rng.standard_normal(x_shape).astype(np.float32)
    if name == "gaussian":
        return dy * np.float32(0.1), x
    if name == "heavy_tail":
        dy = (np.sign(dy) * np.exp2(rng.uniform(-35.0, -20.0, dy_shape))).astype(np.float32)
        flat = dy.reshape(-1)
        flat[flat.size // 3] = np.float32(0.97)
        flat[(2 * flat.size) // 3 + 1] = np.float32(-1.21)
        return dy, np.maximum(x, np.float32(0))
    if name == "small_times_large":
        return dy * np.float32(1e-7), x * np.float32(3e3)
    raise KeyError(name)
