"""Operator cases of the training diagnostics, shared by the host test (tests/test_train_stats_cpu.py) and the device test
(tests/test_gpu_train_stats.py); tests/train_stats_ref.py is the reference of both.  Small on purpose: the row counts straddle the
wave (64) and the workgroup (256), 28 * 28 = 784 pixels is no multiple of 256, and every rule has a case of its own."""
import numpy as np

DENORM = np.float32(1.4e-45)          # the smallest positive float32 denormal (bit pattern 1)
BIG = np.float32(1.0e6)               # fills the delta columns: read as a logit it would win every argmax


def round16(v):
    return (v + 15) // 16 * 16


def _box(name, pred, cls, K, sampled=None):
    return dict(name=name, pred=np.ascontiguousarray(pred, np.float32), cls=np.ascontiguousarray(cls, np.int32), K=K,
                cs=pred.shape[1], sampled=None if sampled is None else np.ascontiguousarray(sampled, np.int32))


def _rows(rng, n, K, lo=-1):
    cs = round16(5 * K + 1)
    pred = np.full((n, cs), BIG, np.float32)                      # deltas and padding: large values that must not be read as logits
    pred[:, :K + 1] = rng.integers(-8, 9, (n, K + 1)).astype(np.float32) * np.float32(0.25)       # a coarse grid: ties are frequent
    return pred, rng.integers(lo, K + 1, n).astype(np.int32)


def box_cases():
    rng = np.random.default_rng(11)
    out = []
    for K in (1, 3, 8):
        for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, 1025)):
            pred, cls = _rows(rng, n, K)
            sampled = rng.integers(0, 300, (1 + i % 3, 2)) if i % 2 == 0 else None          # with and without the sampled counts
            out.append(_box(f"K{K}-rows{n}-{'counts' if sampled is not None else 'nocounts'}", pred, cls, K, sampled))
    K = 3
    pred, _ = _rows(rng, 257, K)
    out.append(_box("all-empty", pred, np.full(257, -1), K))
    out.append(_box("all-background", pred, np.full(257, K), K, [[0, 257]]))
    out.append(_box("all-foreground", pred, rng.integers(0, K, 257), K, [[200, 0], [57, 0]]))
    out.append(_box("labels-minus2-and-K+1-ignored", pred, np.where(np.arange(257) % 2 == 0, -2, K + 1), K))
    tie = np.full((4, 16), BIG, np.float32)
    tie[:, :4] = [[2, 1, 2, 0], [2, 1, 2, 0], [0, 3, 1, 3], [0, 3, 1, 3]]       # rows 0/1: classes 0 and 2 tie; rows 2/3: class 1 and background tie
    out.append(_box("ties-first-index-wins", tie, [0, 2, 1, 3], K))            # -> pred 0, 0, 1, 1
    zero = np.full((3, 16), BIG, np.float32)
    zero[:, :4] = [[-0.0, 0.0, -1, -1], [0.0, -0.0, -1, -1], [-1, -0.0, -1, 0.0]]      # -0.0 == +0.0: the first of them wins
    out.append(_box("signed-zeros-tie", zero, [0, 1, 3], K))
    last = np.full((5, 16), BIG, np.float32)
    last[:, :4] = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [-3, -2, -1, -0.5], [DENORM, 0, -DENORM, 2 * DENORM]]
    out.append(_box("maximum-in-the-last-logit", last, [3, 0, 2, 1, 0], K))
    inf = np.full((3, 16), BIG, np.float32)
    inf[:, :4] = [[-np.inf, -np.inf, -np.inf, -np.inf], [1, np.inf, np.inf, 0], [-np.inf, -1e30, -np.inf, -1e38]]
    out.append(_box("infinities", inf, [0, 2, 1], K))
    return out


def _mask(name, logits, targets, cls, ptr=None):
    side = int(round(np.sqrt(logits.shape[1])))
    return dict(name=name, logits=np.ascontiguousarray(logits, np.float32), targets=np.ascontiguousarray(targets, np.uint8),
                cls=np.ascontiguousarray(cls, np.int32), ptr=ptr, side=side, cs=logits.shape[2], n_masks=logits.shape[0])


SPECIAL = np.array([0.0, -0.0, DENORM, -DENORM, 1e-30, -1e-30, np.inf, -np.inf], np.float32)


def mask_cases():
    rng = np.random.default_rng(12)
    out = []

    def rand(n, side, cs=16):
        lg = rng.standard_normal((n, side * side, cs)).astype(np.float32)
        return lg, rng.integers(0, 2, (n, side * side)).astype(np.uint8)
    for n in (0, 1, 2, 3, 5):
        lg, tg = rand(n, 28)
        out.append(_mask(f"side28-{n}-entries", lg, tg, rng.integers(0, 8, n)))
    lg, tg = rand(1, 2)
    out.append(_mask("side2-1-entry", lg, tg, [3]))
    lg, tg = rand(3, 28)
    for ptr in (2, 3, 7, 0):
        out.append(_mask(f"count-{ptr}-of-capacity-3", lg, tg, [1, 0, 2], ptr=ptr))
    out.append(_mask("classes-0-7-and-invalid-16", lg, tg, [0, 7, 16]))
    out.append(_mask("class-minus1-skipped", lg, tg, [-1, 15, 4]))
    sp = np.tile(SPECIAL, 98)[None, :, None].repeat(2, 0).repeat(16, 2).astype(np.float32)       # 784 = 98 * 8 pixels per entry
    for nm, tg in (("targets-0", np.zeros((2, 784))), ("targets-1", np.ones((2, 784))), ("targets-mixed", rng.integers(0, 2, (2, 784)) * 255)):
        out.append(_mask(f"special-logits-{nm}", sp, tg, [0, 7]))
    return out


def label_cases():
    rng = np.random.default_rng(13)
    return [dict(name=f"len{n}", labels=rng.integers(-1, 2, n).astype(np.int32)) for n in (1, 63, 64, 65, 4097)]
