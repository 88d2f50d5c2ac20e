"""numpy restatements of the two stem-backward kernels (csrc/stem_bwd.hip), for tests/test_freeze_at_cpu.py and
tests/test_gpu_freeze_at.py.  Tensors here are NHWC without halo."""
import numpy as np


def pooled_size(h: int) -> int:
    """Output size of max_pool2d(kernel 3, stride 2, padding 1) along one axis."""
    return (h - 1) // 2 + 1


def pool_argmax(x: np.ndarray) -> np.ndarray:
    """Argmax of every 3x3 stride-2 pad-1 window of x [n][h][w][c] as a flat input index iy * w + ix, [n][hq][wq][c], by ATen's rule
    (max_pool2d_with_indices): the window is scanned in (row, column) order, a later element replaces the current one only if it is
    strictly greater or NaN, and padding positions never take part."""
    n, h, w, c = x.shape
    hq, wq = pooled_size(h), pooled_size(w)
    idx = np.full((n, hq, wq, c), -1, np.int64)
    best = np.zeros((n, hq, wq, c), x.dtype)
    for oy in range(hq):
        for ox in range(wq):
            for iy in range(2 * oy - 1, 2 * oy + 2):
                for ix in range(2 * ox - 1, 2 * ox + 2):
                    if not (0 <= iy < h and 0 <= ix < w):
                        continue
                    v = x[:, iy, ix, :]
                    cur, b = idx[:, oy, ox, :], best[:, oy, ox, :]
                    with np.errstate(invalid="ignore"):
                        take = (cur < 0) | (v > b) | np.isnan(v)
                    best[:, oy, ox, :] = np.where(take, v, b)
                    idx[:, oy, ox, :] = np.where(take, iy * w + ix, cur)
    return idx


def maxpool_relu_bwd(x: np.ndarray, dq: np.ndarray) -> np.ndarray:
    """Gradient w.r.t. the pre-ReLU tensor of max_pool2d(relu(.), 3, 2, 1), given x = the post-ReLU tensor [n][h][w][c] and dq, the
    gradient of the pooled map [n][hq][wq][c]: every pixel sums, in fp32 and in ascending (oy, ox) order, the dq of the windows whose
    argmax it is, then the ReLU mask x > 0 is applied.  The result is float32 (an fp16 kernel rounds it once)."""
    n, h, w, c = x.shape
    idx = pool_argmax(x)
    hq, wq = idx.shape[1:3]
    assert dq.shape == (n, hq, wq, c), (dq.shape, idx.shape)
    acc = np.zeros((n, h * w, c), np.float32)
    nn, cc = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
    for oy in range(hq):                      # ascending (oy, ox): a pixel's windows are added in this order
        for ox in range(wq):
            acc[nn, idx[:, oy, ox, :], cc] += dq[:, oy, ox, :].astype(np.float32)
    return np.where(x.reshape(n, h * w, c) > 0, acc, np.float32(0)).reshape(n, h, w, c).astype(np.float32)


STEM_KPAD = 256          # 7 tap rows x (8 taps x 4 channels), padded to 256 columns


def stem_wgrad(dy: np.ndarray, x0: np.ndarray, scale=None) -> np.ndarray:
    """float64 weight gradient of the 7x7 stride-2 pad-3 stem convolution in its forward GEMM layout [64][256], column
    (kh * 8 + kw) * 4 + ci: grad[co][kh][kw][ci] = scale[co] * sum_{n,y,x} dy[n][y][x][co] * x0[n][2y+kh-3][2x+kw-3][ci].
    dy [n][hc][wc][co], x0 [n][2 hc][2 wc][cin] (cin <= 4).  The padding columns are zero.  Also returns, as the second value, the
    same sum over |dy| |x0| (the scale of a rounding bound)."""
    n, hc, wc, co = dy.shape
    cin = x0.shape[3]
    assert x0.shape[:3] == (n, 2 * hc, 2 * wc) and cin <= 4
    xp = np.zeros((n, 2 * hc + 6, 2 * wc + 6, cin), np.float64)
    xp[:, 3:-3, 3:-3] = x0
    d = dy.astype(np.float64).reshape(-1, co)
    g = np.zeros((co, 7, 8, 4), np.float64)
    a = np.zeros((co, 7, 8, 4), np.float64)
    for kh in range(7):
        for kw in range(7):
            win = xp[:, kh:kh + 2 * hc:2, kw:kw + 2 * wc:2, :].reshape(-1, cin)
            g[:, kh, kw, :cin] = d.T @ win
            a[:, kh, kw, :cin] = np.abs(d).T @ np.abs(win)
    if scale is not None:
        g *= np.asarray(scale, np.float64)[:, None, None, None]
        a *= np.abs(np.asarray(scale, np.float64))[:, None, None, None]
    out = np.zeros((co, STEM_KPAD), np.float64)
    mag = np.zeros((co, STEM_KPAD), np.float64)
    out[:, :224] = g.reshape(co, 224)
    mag[:, :224] = a.reshape(co, 224)
    return out, mag


def stem_padding_mask() -> np.ndarray:
    """True for the padding columns of the stem's [256]-column layout given 4 stored channels: the eighth tap of every row and the
    columns from 224 on (the padding channels of a 3-band model are ``column % 4 >= 3``, added by the caller)."""
    col = np.arange(STEM_KPAD)
    return (col >= 224) | ((col >> 2) & 7 == 7)
