"""The optimiser step of csrc/sgd_rule.h restated in numpy -- once in fp32, operation for operation (numpy rounds every product and sum
on its own, as the kernel does), and once in float64 -- plus the norms and clipping coefficients in float64, the bounds the tests
hold the kernels to, and the synthetic segment tables they run on.  torch on the CPU pins both restatements
(tests/test_solver_cpu.py); the GPU tests compare the kernels against the float64 one (tests/test_gpu_solver.py).

    g = grad * inv_scale;  g = clip(g);  g += wd * w;  b = mu * buf + g;  d = nesterov ? g + mu * b : b;  w -= lr * d;  buf = b
"""
import numpy as np

CHUNK = 8192                     # csrc/sgd_rule.h SGD_CHUNK
U21, U22 = 2.0 ** -21, 2.0 ** -22


def rule(w, buf, grad, inv_scale, lr, wd, mu, nesterov, clamp=None, coef=1.0, dtype=np.float32):
    """One step on arrays of one segment; every scalar is first rounded to fp32 (the C ABI's type), then the arithmetic runs in
    ``dtype``.  ``clamp``: value clipping to +-clamp; otherwise the gradient is multiplied by ``coef``.  Returns (w, buf)."""
    f = lambda x: np.asarray(np.float32(x)).astype(dtype)                       # noqa: E731
    w, buf, grad = (np.asarray(a, np.float32).astype(dtype) for a in (w, buf, grad))
    g = grad * f(inv_scale)
    g = np.clip(g, -f(clamp), f(clamp)) if clamp is not None else g * np.asarray(coef, np.float32).astype(dtype)
    g = g + f(wd) * w
    b = f(mu) * buf + g
    d = g + f(mu) * b if nesterov else b
    return w - f(lr) * d, b


def norms64(grad, inv_scale, segs, norm_type=2.0):
    """float64 norm of grad * inv_scale over every (offset, count, flag) segment."""
    out = []
    for off, cnt, _ in segs:
        u = np.asarray(grad[off:off + cnt], np.float64) * float(np.float32(inv_scale))
        out.append(np.abs(u).max() if np.isinf(norm_type) else np.sqrt(np.sum(u * u)))
    return np.array(out, np.float64)


def total64(norms, norm_type=2.0):
    return norms.max() if np.isinf(norm_type) else np.sqrt(np.sum(norms * norms))


def coef64(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), in float64."""
    return np.minimum(1.0, float(np.float32(max_norm)) / (np.asarray(norm, np.float64) + 1e-6))


def coef32(norm, max_norm):
    """The same in the fp32 arithmetic torch and the kernel use, from an fp32 norm."""
    return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.asarray(norm, np.float32) + np.float32(1e-6))).astype(np.float32)


def bounds(w, buf, grad, inv_scale, lr, wd, mu, clamp=None, coef=1.0):
    """Per-element bounds (for w, for buf) on |fp32 result - float64 rule|: 2^-21 times the sum of the magnitudes the partial results
    are bounded by -- at most ten fp32 roundings of half an ulp each, every one of a partial result no larger than its share of
    |w| + lr (1 + mu) (mu |buf| + |g~| + wd |w|), where g~ is the clipped gradient.  Counted out: their sum stays below 8 half-ulps of
    that sum for mu <= 1."""
    w, buf, grad = (np.abs(np.asarray(a, np.float64)) for a in (w, buf, grad))
    g = grad * float(np.float32(inv_scale))
    g = np.minimum(g, float(np.float32(clamp))) if clamp is not None else g * np.asarray(coef, np.float64)
    lr, wd, mu = (float(np.float32(x)) for x in (lr, wd, mu))
    t = mu * buf + g + wd * w
    return U21 * (w + lr * (1.0 + mu) * t), U21 * t


def table(counts, gaps, lead=8, tail=7):
    """Segments of ``counts`` values, segment i preceded by ``gaps[i % len(gaps)]`` free values beyond the next multiple of 4, the first
    by ``lead``; ``tail`` free values at the end.  Returns ([(offset, count, flag)], n); flags alternate weight / bias."""
    segs, pos = [], lead
    for i, c in enumerate(counts):
        if i:
            pos = (pos + 3) // 4 * 4 + gaps[i % len(gaps)]
        segs.append((pos, int(c), i & 1))
        pos += int(c)
    return segs, pos + tail


def gradients(rng, segs, n, inv_scale, max_norm, zero_segment, norm_type=2.0):
    """A gradient buffer whose segments alternate between half and twice ``max_norm`` (in ``norm_type``, after inv_scale), segment ``zero_segment``
    all zero, and the gaps filled too (today's step updates them)."""
    g = (rng.standard_normal(n) / np.float32(inv_scale) * 0.01).astype(np.float32)
    for i, (off, cnt, _) in enumerate(segs):
        v = rng.standard_normal(cnt)
        size = np.abs(v).max() if np.isinf(norm_type) else np.sqrt(np.sum(v * v))
        v *= (0.5 if i % 3 == 0 else 2.0) * max_norm / max(size, 1e-30) / float(np.float32(inv_scale))
        g[off:off + cnt] = 0.0 if i == zero_segment else v.astype(np.float32)
    return g


def step64(w, buf, grad, segs, inv_scale, lr, mu, wd, nesterov=False, bias_lr_factor=1.0, wd_bias=None, clip="none", clip_value=1.0, coef=None):
    """The whole segmented step in float64 on copies: values outside every segment take lr, wd and no clipping.  ``coef``: the
    per-segment coefficients to use for "norm" / "full_model" (the kernel's own, read back).  Returns (w, buf, tol_w, tol_buf)."""
    w0, b0, g0 = (np.asarray(a, np.float32) for a in (w, buf, grad))
    gap = np.ones(len(w0), bool)
    for off, cnt, _ in segs:
        gap[off:off + cnt] = False
    w1, b1, tw, tb = (np.zeros(len(w0), np.float64) for _ in range(4))
    w1[gap], b1[gap] = rule(w0[gap], b0[gap], g0[gap], inv_scale, lr, wd, mu, nesterov, dtype=np.float64)
    tw[gap], tb[gap] = bounds(w0[gap], b0[gap], g0[gap], inv_scale, lr, wd, mu)
    lr_b = np.float32(lr) * np.float32(bias_lr_factor)
    for i, (off, cnt, flag) in enumerate(segs):
        s = slice(off, off + cnt)
        kw = dict(clamp=clip_value) if clip == "value" else dict(coef=1.0 if coef is None else coef[i])
        lr_s, wd_s = (lr_b, wd if wd_bias is None else wd_bias) if flag else (lr, wd)
        w1[s], b1[s] = rule(w0[s], b0[s], g0[s], inv_scale, lr_s, wd_s, mu, nesterov, dtype=np.float64, **kw)
        tw[s], tb[s] = bounds(w0[s], b0[s], g0[s], inv_scale, lr_s, wd_s, mu, **kw)
    return w1, b1, tw, tb
