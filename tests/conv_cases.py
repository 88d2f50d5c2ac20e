"""The case grid of the convolution operators (rs_op_conv2d, rs_op_conv2d_split, rs_op_conv2d_dual, rs_op_conv2d_dgrad, rs_op_bneck_tail,
rs_op_bneck_tail_split), shared by tools/parity/conv_op_compare.py (which hashes the outputs of two builds) and by the tests that hold
those outputs to a float64 reference (tests/test_gpu_conv_bounds.py on the GPU, tests/test_conv_bounds_cpu.py on an emulation); the
float64 reference with its per-element error bound; and the check of an output buffer against them.  Nothing here needs a GPU.

The bound.  A(K) = 2e-7 sqrt(K) + 1e-6 is the project's allowance for an fp32-accumulating chain of K products, in units of
s = |terms|_2 + |bias| + |addends| of the element (TOL of tests/test_gpu_split.py).  The fp16 kernels accumulate in fp32 and round once,
after the fp32 epilogue:
    fp16 out          A s + 2^-11 (|ref| + A s) + 2^-25      accumulation noise, half an fp16 ulp of the value that is rounded, subnormal floor
    fp32 out, fp16    A s + 2^-24 |ref|
    split mode        A(K) s
with, for the fp16 kernels, A = allowance(K) = max(A(K), 1.5 x the err / s the fp32-MFMA mode reached on fp16-representable operands of that depth:
F32_MODE_ERR below, measured, profiles/conv_bounds/README.md)."""
import json
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 13, 11), (2, 24, 20)]
IGEMM = {0: 128, 1: 64, 3: 128, 4: 256, 7: 128, 8: 64, 9: 128, 10: 256, 14: 256}      # variant -> rows must be a multiple of
DEEP_F16, DEEP_SPLIT = [12, 15, 16, 17, 18, 19, 20], [12, 15, 16, 17]
WREG, WIDE = [22, 23, 25, 26], [28, 29, 30, 31]
FC_M = 143                      # rows of the K = 12544 FC, laid out as an (M x 1)-pixel image (tests/test_gpu_conv.py::test_fc_gemm)
SENTINEL = 30000.0              # what the output buffers hold before a run: exact in fp16 and fp32, beyond every reference value's bound


def _variants(split, cin, cout, k, stride, res, up, deconv, train=False, scatter=False):
    rows = cout * (4 if deconv else 1)
    out = [-1] + [v for v, mult in IGEMM.items() if rows % mult == 0]
    if not deconv and rows % 256 == 0 and not scatter:
        out += [12] if train else (DEEP_SPLIT if split else DEEP_F16)
    one_by_one = k == 1 and stride == 1 and cin == 256 and not deconv and not train
    if one_by_one and not split and rows % 256 == 0 and not (res and up):
        out += WREG
    if one_by_one and split and rows % 64 == 0 and not up:
        out += WIDE
    return out


# (case, variant) pairs the library may refuse: {(tag, variant): the RS_CHECK message that justifies it}.  -1 and the variants the engine's
# table launches on the layer class may not stand here (tests/test_gpu_conv_bounds.py asserts it).
EXPECTED_REFUSED = {}


# ---------------------------------------------------------------------------------------------------------------- tags (the tool's hash keys)
def conv_tag(split, n, h, w, cin, cout, k, stride, res, up, relu, deconv=False, out_f32=False):
    return "%s conv%dx%d s%d %d->%d %dx%dx%d%s%s%s%s%s" % ("split" if split else "fp16", k, k, stride, cin, cout, n, h, w, " res" if res else "",
                                                        " up" if up else "", " relu" if relu else "", " deconv" if deconv else "", " f32out" if out_f32 else "")


def dual_tag(n, h, w, cin, cin2, cout, stride2):
    return "fp16 dual 1x1 %d+%d->%d s2=%d %dx%dx%d" % (cin, cin2, cout, stride2, n, h, w)


def dgrad_tag(n, hi, wi, cin, cout, k, stride, res, res32, mask, down):
    return "dgrad %dx%d s%d %d<-%d %dx%dx%d%s%s%s%s" % (k, k, stride, cin, cout, n, hi, wi, " res" if res else "", " res32" if res32 else "", " mask" if mask else "",
                                                      " down" if down else "")


def deconv_predict_tag(entries, count, side):
    return "split deconv+predict %d of %d entries side %d" % (count, entries, side)


def bneck_tag(split, n, h, w, width, nxt, proj):
    return "%s bneck tail width %d %dx%dx%d%s%s" % ("split" if split else "fp16", width, n, h, w, " next" if nxt else "", " proj" if proj else "")


def tool_cases():
    """The cases of tools/parity/conv_op_compare.py in its order: (method of its Runner, positional arguments, keyword arguments)."""
    out = []
    for split in (False, True):
        for n, h, w in SHAPES:
            for cin in (64, 256):
                for cout in (64, 256, 1024):
                    for k, stride in ((1, 1), (1, 2), (3, 1), (3, 2)):
                        epis = [(False, False, False), (True, False, True), (False, True, True)] if (k, stride) == (1, 1) else [(False, False, True)]
                        if (k, stride, cin, cout) == (3, 1, 256, 256):
                            epis.append((True, True, True))
                        for res, up, relu in epis:
                            out.append(("conv", (split, n, h, w, cin, cout, k, stride, res, up, relu), {}))
            out.append(("conv", (split, n, h, w, 256, 256, 1, 1, False, False, True), {"deconv": True}))             # mode 1
            out.append(("conv", (split, n, h, w, 256, 16, 1, 1, False, False, False), {"out_f32": True}))           # the fp32-out head tile
            for width in (64, 128):
                for nxt in (False, True):
                    out.append(("bneck", (split, n, h, w, width, nxt, False), {}))
                    if width == 64:
                        out.append(("bneck", (split, n, h, w, width, nxt, True), {}))
    for n, h, w in SHAPES:
        out.append(("dual", (n, h, w, 64, 64, 256, 1), {}))
        out.append(("dual", (n, h, w, 256, 256, 1024, 2), {}))
        out.append(("dgrad", (n, h, w, 256, 256, 3, 1, False, True, True, True), {}))
        out.append(("dgrad", (n, h, w, 256, 256, 3, 1, True, False, False, False), {}))
        out.append(("dgrad", (n, h, w, 64, 256, 1, 1, False, True, True, False), {}))
        out.append(("dgrad", (n, h, w, 256, 1024, 1, 2, False, False, True, False), {}))                           # out_stride 2
    out.append(("deconv_predict", (5, 3, 14), {}))
    out.append(("deconv_predict", (9, 9, 7), {}))
    return out


# ---------------------------------------------------------------------------------------------------------------- the engine's layer classes
def stage_class(name, cin2, spec):
    """(stride, epilogue) of a stage of tests.util.conv_stage_shapes by its name, None for a stage with no operator entry of its own
    (the fused stem and tails, the RPN conv with its heads in the epilogue, the fp16 fused mask predictor).  For the dual-source conv3 the
    stride is the second source's."""
    leaf = name.split(".")[-1]
    first_of_stage = name.startswith("res") and name.split(".")[1] == "0" and not name.startswith("res2")
    if "+" in name:
        return None
    if leaf == "conv3":
        return (2 if first_of_stage else 1, "dual") if cin2 else (1, "res_relu")
    if leaf in ("conv1", "conv2"):
        return (2 if first_of_stage and leaf == ("conv1" if spec.stride_in_1x1 else "conv2") else 1), "relu"
    if name in ("fpn_lateral2", "fpn_lateral3", "fpn_lateral4"):
        return 1, "up"
    if name == "fpn_lateral5" or name == "fpn_output2-5":
        return 1, "none"
    if leaf in ("fc1", "fc2") or leaf.startswith("fcn"):
        return 1, "relu"
    if name == "box.predictor":
        return 1, "f32out"
    return None


def engine_classes():
    """The distinct (cin, k, stride, cout, cin2, epilogue, variant) the fp16 engine launches: every stage of the default spec joined with the
    tile table tests/golden/conv_variants.json at its four batch sizes.  Variants 13 and 21 (fused tails, fused stem) have their own tests."""
    from proj_roadsurf_amd.spec import EngineSpec
    from tests.util import conv_stage_shapes
    spec = EngineSpec()
    with open(os.path.join(ROOT, "tests", "golden", "conv_variants.json")) as f:
        golden = json.load(f)
    table = golden["variants"]
    out = []
    for name, _pix, cin, k, cout, cin2, _forced in conv_stage_shapes(spec, *golden["net_input"]):
        cls = stage_class(name, cin2, spec)
        if cls is None:
            continue
        for v in table[name]:
            if v in (13, 21):
                continue
            t = (cin, k, cls[0], cout, cin2, cls[1], v)
            if t not in out:
                out.append(t)
    return out


class Case:
    """One operator call: the operator, its geometry and epilogue, the variants to run and those that must not be refused."""
    _defaults = dict(op="conv", tag="", split=False, n=1, h=1, w=1, cin=64, cout=64, k=1, stride=1, res=False, up=False, relu=False, deconv=False, out_f32=False,
                     cin2=0, stride2=1, res32=False, mask=False, down=False, in_halo=None, out_halo=1, rows_real=None, variants=(-1,), required=(-1,),
                     width=64, nxt=False, proj=False, w2_mean=0.25, flag_limit=0.05)

    def __init__(self, **kw):
        for key, val in self._defaults.items():
            setattr(self, key, kw.pop(key, val))
        assert not kw, kw
        assert set(self.required) <= set(self.variants), self.tag

    def __repr__(self):
        return self.tag


def _class_variants():
    """layer class (cin, k, stride, cout, cin2, epilogue) -> variants of the engine's table"""
    out = {}
    for t in engine_classes():
        out.setdefault(t[:6], []).append(t[6])
    return out


def _epi_name(res, up, relu, out_f32):
    return "f32out" if out_f32 else "res_relu" if (res and relu and not up) else "up" if (up and not res and not relu) else "relu" if (relu and not res and not up) else \
        "none" if not (res or up or relu) else "other"


def bound_cases():
    """Every case the tests run: the tool's grid (every variant _variants() admits; without the fused deconv + predictor, which
    tests/test_gpu_split_wide1x1.py holds to float64) and the engine's layer classes the grid lacks (the tabled variants and -1)."""
    classes = _class_variants()
    out, seen = [], set()
    for kind, a, kw in tool_cases():
        if kind == "conv":
            split, n, h, w, cin, cout, k, stride, res, up, relu = a
            deconv, out_f32 = kw.get("deconv", False), kw.get("out_f32", False)
            key = (cin, k, stride, cout, 0, _epi_name(res, up, relu, out_f32))
            tabled = [] if (split or deconv) else classes.get(key, [])
            if not (split or deconv):
                seen.add(key)
            variants = [-1, 2] if out_f32 else _variants(split, cin, cout, k, stride, res, up, deconv)
            out.append(Case(op="conv", tag=conv_tag(*a, **kw), split=split, n=n, h=h, w=w, cin=cin, cout=cout, k=k, stride=stride, res=res, up=up, relu=relu,
                            deconv=deconv, out_f32=out_f32, rows_real=15 if out_f32 else None, variants=tuple(variants), required=tuple([-1] + tabled)))
        elif kind == "dual":
            n, h, w, cin, cin2, cout, stride2 = a
            key = (cin, 1, stride2, cout, cin2, "dual")
            seen.add(key)
            out.append(Case(op="dual", tag=dual_tag(*a), n=n, h=h, w=w, cin=cin, cin2=cin2, cout=cout, stride2=stride2, relu=True, in_halo=0,
                            variants=tuple([-1] + [v for v, mult in IGEMM.items() if cout % mult == 0]), required=tuple([-1] + classes.get(key, []))))
        elif kind == "dgrad":
            n, hi, wi, cin, cout, k, stride, res, res32, mask, down = a
            out.append(Case(op="dgrad", tag=dgrad_tag(*a), n=n, h=hi, w=wi, cin=cin, cout=cout, k=k, stride=stride, res=res, res32=res32, mask=mask, down=down,
                            variants=tuple(_variants(False, cout, cin, k, 1, False, False, False, train=True, scatter=stride > 1))))
        elif kind == "bneck":
            split, n, h, w, width, nxt, proj = a
            out.append(Case(op="bneck", tag=bneck_tag(*a), split=split, n=n, h=h, w=w, width=width, nxt=nxt, proj=proj))
    # the fp16 tails once more on conv2 weights of zero mean, as every other operand here is drawn (build_bneck says why the grid's tails are not)
    for width in (64, 128):
        n, h, w = SHAPES[1]
        out.append(Case(op="bneck", tag=bneck_tag(False, n, h, w, width, True, False) + " zero-mean w2", n=n, h=h, w=w, width=width, nxt=True,
                        w2_mean=0.0, flag_limit=0.10))
    for key, tabled in classes.items():
        if key in seen:
            continue
        cin, k, stride, cout, cin2, epi = key
        shapes = [(1, FC_M, 1)] if cin * k * k > 10000 else SHAPES
        for n, h, w in shapes:
            fc = (n, h, w) == (1, FC_M, 1)
            tag = "fp16 class conv%dx%d s%d %d%s->%d %s %dx%dx%d" % (k, k, stride, cin, "+%d" % cin2 if cin2 else "", cout, epi, n, h, w)
            common = dict(tag=tag, n=n, h=h, w=w, cin=cin, cout=cout, variants=tuple([-1] + tabled), required=tuple([-1] + tabled))
            if epi == "dual":
                out.append(Case(op="dual", cin2=cin2, stride2=stride, relu=True, in_halo=0, **common))
            else:
                out.append(Case(op="conv", k=k, stride=stride, res=epi == "res_relu", up=epi == "up", relu=epi in ("relu", "res_relu"), out_f32=epi == "f32out",
                                rows_real=15 if epi == "f32out" else None, in_halo=0 if fc else None, out_halo=0 if fc else 1, **common))
    return out


# ---------------------------------------------------------------------------------------------------------------- bound
def A(k):
    return 2e-7 * np.sqrt(k) + 1e-6


# K -> the largest err / s of the fp32-MFMA mode (use_glds = -1, csrc/ref_f32.hip) on the fp16-representable operands of one case of that depth,
# measured on the MI355X (profiles/conv_bounds/README.md).
F32_MODE_ERR = {64: 7.30e-7, 256: 1.83e-6, 576: 4.29e-6, 2304: 7.70e-6, 4608: 1.34e-5, 12544: 1.69e-5}


def allowance(k):
    """max(A(K), 1.5 x the fp32 mode's measured err / s): for a depth between two measured ones the measurement of the next SMALLER depth
    counts (the noise grows with K, so that is never the wider choice)."""
    m = max([v for kk, v in F32_MODE_ERR.items() if kk <= k], default=0.0)
    return max(A(k), 1.5 * m)


def bound(mode, k, ref, s):
    """mode: 'f16' (fp16 out), 'f16_f32out', 'split'"""
    if mode == "split":         # as tests/test_gpu_split.py holds these kernels: A(K) itself, not widened by the fp32 mode's measurement
        return A(k) * s
    a = allowance(k) * s
    if mode == "f16":
        return a + 2.0 ** -11 * (np.abs(ref) + a) + 2.0 ** -25
    assert mode == "f16_f32out"
    return a + 2.0 ** -24 * np.abs(ref)


# ---------------------------------------------------------------------------------------------------------------- operands
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _planes(a32):
    hi = a32.astype(np.float16)
    return np.stack([hi, (a32 - hi.astype(np.float32)).astype(np.float16)])


def _val(planes):
    return planes[0].astype(np.float64) + planes[1].astype(np.float64)


def _haloed(a, halo):
    if halo == 0:
        return np.ascontiguousarray(a)
    n, h, w, c = a.shape
    out = np.zeros((n, h + 2 * halo, w + 2 * halo, c), a.dtype)
    out[:, halo:halo + h, halo:halo + w] = a
    return out


def _spread_act(rng, n, h, w, c):
    """activations whose channels are spread over decades: N(0,1) x exp(1.5 N(0,1)) per channel, |x| <= 1000"""
    x = rng.standard_normal((n, h, w, c)) * np.exp(1.5 * rng.standard_normal(c))
    return np.clip(x, -1000.0, 1000.0).astype(np.float32)


def _spread_weight(rng, rows, k, mean=0.0):
    """rows spread by exp(N(0,1)) around 1 / sqrt(K)"""
    return ((rng.standard_normal((rows, k)) + mean) / np.sqrt(k) * np.exp(rng.standard_normal(rows))[:, None]).astype(np.float32)


def _addend(rng, n, h, w, c):
    return (4.0 * rng.standard_normal((n, h, w, c))).astype(np.float32)


class Problem:
    """Operands in the layout the operator takes (numpy, with halos), the float64 reference and bound over the output's interior
    [n][OH][OW][stored channels], and which interior pixels the kernel writes at all (a strided input gradient leaves the others alone)."""


def _stored(a32, split):
    """(what the device gets, the float64 values it stands for)"""
    if split:
        p = _planes(a32)
        return p, _val(p)
    h = a32.astype(np.float16)
    return h, h.astype(np.float64)


def _patches(xv, k, stride, pad, halo, ho, wo):
    """im2col in the kernels' K order (tap row, tap column, channel) of a haloed [n][H + 2 halo][W + 2 halo][C] float64 map"""
    o = halo - pad
    return np.concatenate([xv[:, o + i:o + i + stride * (ho - 1) + 1:stride, o + j:o + j + stride * (wo - 1) + 1:stride] for i in range(k) for j in range(k)], -1)


def build(case):
    """Draw the operands of a conv / dual / dgrad case (seeded by its tag, separate from the tool's) and compute reference and bound."""
    from proj_roadsurf_amd.weights import split_planes
    c = case
    rng = _rng("bounds " + c.tag)
    P = Problem()
    P.case, split = c, c.split
    if c.op == "dgrad":
        # the input gradient as the forward convolution it is: dy [n][ho][wo][cout] -> dx [n][hi][wi][cin] at every stride-th pixel
        ho, wo = (c.h, c.w) if c.stride == 1 else ((c.h + c.stride - 1) // c.stride, (c.w + c.stride - 1) // c.stride)
        gin, gout, pad, in_halo, conv_stride, out_stride = c.cout, c.cin, c.k - 1 - c.k // 2, 1, 1, c.stride
        ih, iw = ho, wo
    else:
        pad = c.k // 2
        in_halo = pad if c.in_halo is None else c.in_halo
        gin, gout, conv_stride, out_stride = c.cin, c.cout, c.stride, 1
        ih, iw = c.h, c.w
        ho, wo = (ih + 2 * pad - c.k) // c.stride + 1, (iw + 2 * pad - c.k) // c.stride + 1
    P.pad, P.in_halo, P.ho, P.wo = pad, in_halo, ho, wo
    nrows = gout * (4 if c.deconv else 1)
    rows_real = c.rows_real or nrows
    kdim = c.k * c.k * gin + c.cin2
    P.K = kdim
    P.x, xv = _stored(_haloed(_spread_act(rng, c.n, ih, iw, gin), in_halo), split)
    pt = _patches(xv, c.k, conv_stride, pad, in_halo, ho, wo)
    if c.op == "dual":
        P.x2, x2v = _stored(_haloed(_spread_act(rng, c.n, c.h * c.stride2, c.w * c.stride2, c.cin2), 1), False)
        pt = np.concatenate([pt, x2v[:, 1:1 + c.stride2 * (ho - 1) + 1:c.stride2, 1:1 + c.stride2 * (wo - 1) + 1:c.stride2]], -1)
    pt = pt.reshape(-1, kdim)
    w32 = _spread_weight(rng, nrows, kdim)
    w32[rows_real:] = 0
    bias = rng.standard_normal(nrows).astype(np.float32)
    bias[rows_real:] = 0
    if c.op == "dgrad":
        bias[:] = 0                                 # the operator has none
    P.bias = bias
    if split:
        P.w, P.wscale = split_planes(w32)
        wv = (P.w[:nrows].astype(np.float64) + P.w[nrows:].astype(np.float64)) * P.wscale.astype(np.float64)[:, None]
    else:
        P.w = w32.astype(np.float16)
        wv = P.w.astype(np.float64)
    acc = pt @ wv.T
    s = np.sqrt((pt * pt) @ (wv * wv).T)
    del pt
    if c.deconv:            # rows (dy, dx, co) -> pixel (2 y + dy, 2 x + dx)
        shuffle = lambda a: a.reshape(c.n, ho, wo, 2, 2, gout).transpose(0, 1, 3, 2, 4, 5).reshape(c.n, 2 * ho, 2 * wo, gout)
        ref, s = shuffle(acc + bias.astype(np.float64)), shuffle(s + np.abs(bias.astype(np.float64)))
    else:
        ref = (acc + bias.astype(np.float64)).reshape(c.n, ho, wo, nrows)
        s = (s + np.abs(bias.astype(np.float64))).reshape(c.n, ho, wo, nrows)
    oh, ow = ref.shape[1:3]
    P.res = P.up = P.res32 = P.mask = P.down = None
    sy, sx = slice(0, out_stride * (oh - 1) + 1, out_stride), slice(0, out_stride * (ow - 1) + 1, out_stride)      # where an output pixel lands in the map of the addends
    fh, fw = (c.h, c.w) if c.op == "dgrad" else (oh, ow)                                                              # that map's size
    if c.res:
        P.res, v = _stored(_haloed(_addend(rng, c.n, fh, fw, gout), 1), split)
        v = v[:, 1:-1, 1:-1][:, sy, sx]
        ref, s = ref + v, s + np.abs(v)
    if c.up:                # the coarser map at (y / 2, x / 2); an odd edge reads its (zero) halo
        P.up, v = _stored(_haloed(_addend(rng, c.n, oh // 2, ow // 2, gout), 1), split)
        v = v[:, 1 + np.arange(oh) // 2][:, :, 1 + np.arange(ow) // 2]
        ref, s = ref + v, s + np.abs(v)
    if c.down:              # the 2 x 2 block of the finer map
        P.down, v = _stored(_haloed(_addend(rng, c.n, 2 * oh, 2 * ow, gout), 1), False)
        v = v[:, 1:-1, 1:-1].reshape(c.n, oh, 2, ow, 2, gout)
        ref, s = ref + v.sum((2, 4)), s + np.abs(v).sum((2, 4))
    if c.res32:
        P.res32 = _haloed(_addend(rng, c.n, fh, fw, gout), 1)
        v = P.res32.astype(np.float64)[:, 1:-1, 1:-1][:, sy, sx]
        ref, s = ref + v, s + np.abs(v)
    if c.mask:
        P.mask, v = _stored(_haloed(rng.standard_normal((c.n, fh, fw, gout)).astype(np.float32), 1), False)
        ref = np.where(v[:, 1:-1, 1:-1][:, sy, sx] > 0, ref, 0.0)
    if c.relu:
        ref = np.maximum(ref, 0.0)
    mode = "split" if split else ("f16_f32out" if c.out_f32 else "f16")
    bnd = bound(mode, kdim, ref, s)
    # scattered to the output map
    P.oh, P.ow = (c.h, c.w) if c.op == "dgrad" else (oh, ow)
    P.written = np.zeros((c.n, P.oh, P.ow), bool)
    P.written[:, sy, sx] = True
    P.ref = np.zeros((c.n, P.oh, P.ow, nrows if not c.deconv else gout))
    P.bound = np.zeros_like(P.ref)
    P.s = np.ones_like(P.ref)
    P.ref[:, sy, sx], P.bound[:, sy, sx], P.s[:, sy, sx] = ref, bnd, s
    P.rows_real, P.mode = rows_real, mode
    P.out_halo = c.out_halo
    P.planes = 2 if (split and not c.out_f32) else 1
    P.out_dtype = np.float32 if c.out_f32 else np.float16
    check_reference(P)
    return P


def check_reference(P):
    """What the bound presumes, on the reference alone: the fp16 clamp is never reached, and a pixel that keeps the sentinel cannot pass."""
    assert np.all(np.abs(P.ref) < 60000.0), "reference reaches the fp16 clamp"
    unwritten = SENTINEL * P.planes
    assert np.all(np.abs(unwritten - P.ref) > 2.0 * P.bound + 1.0), "an unwritten element could pass the bound"


def empty_output(P):
    """the output buffer as it is before the run: the sentinel everywhere, both planes in the split mode"""
    shape = (P.ref.shape[0], P.oh + 2 * P.out_halo, P.ow + 2 * P.out_halo, P.ref.shape[3])
    return np.full(((2,) + shape) if P.planes == 2 else shape, SENTINEL, P.out_dtype)


def sentinel_filled(shape, dtype, dev):
    """an output buffer as the operator tests hand it to a kernel (a torch tensor on `dev`): the sentinel in every element, so that what a kernel
    leaves alone is told from what it wrote, zeros included"""
    import torch
    return torch.full(shape, SENTINEL, dtype=dtype, device=dev)


def _host(o):
    return o if isinstance(o, np.ndarray) else o.numpy()


def untouched(o):
    """per element of a buffer back on the host (numpy array or torch tensor, fp16 or fp32): does it still hold the sentinel, bit for bit"""
    a = _host(o)
    return _bits(a) == _bits(np.array([SENTINEL], a.dtype))[0]


def assert_halo_untouched(o, halo, what="kernel wrote into the halo"):
    """o [...][H + 2 halo][W + 2 halo][C]: every halo element still holds the sentinel"""
    a = _host(o)
    keep = np.ones(a.shape, bool)
    keep[..., halo:a.shape[-3] - halo, halo:a.shape[-2] - halo, :] = False
    bad = int((~untouched(a))[keep].sum())
    assert bad == 0, f"{what}: {bad} elements"


def assert_all_untouched(o, what):
    """a buffer that is none of the kernel's business: the sentinel in every element"""
    assert bool(untouched(o).all()), what


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def interior(P, buf):
    h = P.out_halo
    return buf[..., h:h + P.oh, h:h + P.ow, :]


def check_output(P, buf):
    """Every element of the buffer a run left behind: the halo and the interior pixels the kernel does not own bit for bit the sentinel, every
    other element inside its bound, padded head rows equal to their zero bias.  Returns the largest err / bound; raises AssertionError."""
    keep = np.ones(buf.shape, bool)
    interior(P, keep)[...] = False
    interior(P, keep)[..., ~P.written, :] = True
    bad = ~untouched(buf)[keep]
    assert not bad.any(), "%s: %d elements outside the kernel's pixels (halo / unowned) were written" % (P.case.tag, int(bad.sum()))
    got = interior(P, buf).astype(np.float64)
    if P.planes == 2:
        got = got[0] + got[1]
    err = np.abs(got - P.ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(P.written[..., None] & (err != 0), err / P.bound, 0.0)      # err == 0: a padded row (bound 0) or an exact zero
    if P.rows_real < P.ref.shape[3]:
        pad_rows = got[P.written][:, P.rows_real:]
        assert np.all(pad_rows == 0.0), "%s: padded head rows hold something else than their zero bias" % P.case.tag
    worst = float(ratio.max())
    if not worst <= 1.0:        # also catches NaN
        i = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %r, ref %r, bound %r (err / bound %.3f)" % (
            P.case.tag, int((~(ratio <= 1.0)).sum()), ratio.size, i, got[i], P.ref[i], P.bound[i], ratio[i]))
    return worst


# ---------------------------------------------------------------------------------------------------------------- emulation (no GPU)
def emulate(P, x=None):
    """What a correct fp16-mode kernel leaves in the buffer, up to the summation order: fp32 accumulation of the stored operands, the fp32
    epilogue, one rounding to the output type.  conv cases without deconv; x replaces the stored input map (a seeded fault)."""
    c = P.case
    assert c.op == "conv" and not c.split and not c.deconv
    xv = (P.x if x is None else x).astype(np.float32)
    pt = _patches(xv, c.k, c.stride, P.pad, P.in_halo, P.ho, P.wo).reshape(-1, P.K)
    v = (pt @ P.w.astype(np.float32).T + P.bias).reshape(c.n, P.ho, P.wo, -1)
    if c.res:
        v = v + P.res.astype(np.float32)[:, 1:-1, 1:-1]
    if c.up:
        v = v + P.up.astype(np.float32)[:, 1 + np.arange(P.oh) // 2][:, :, 1 + np.arange(P.ow) // 2]
    if c.relu:
        v = np.maximum(v, np.float32(0))
    buf = empty_output(P)
    interior(P, buf)[...] = v.astype(P.out_dtype)
    return buf


# ---------------------------------------------------------------------------------------------------------------- bottleneck tails
def _r16_relu_span(pre, e):
    """fp16(relu(.)) of pre, and by how much it can move when pre moves by up to e: the rounding (or ReLU) boundaries within reach"""
    r = lambda a: np.maximum(a, 0.0).astype(np.float16).astype(np.float64)
    mid = r(pre)
    return mid, np.maximum(np.abs(r(pre + e) - mid), np.abs(r(pre - e) - mid))


def build_bneck(case):
    """rs_op_bneck_tail(_split): t2 = relu(conv3x3(t1)), out = relu(conv1x1(t2) + identity x | projection of x0), t1n = relu(conv1x1(out)), chained
    through registers.  fp16: t2 and out are rounded to fp16 on the way, so the reference rounds them too, and an element of t2 (out) whose
    value lies within its accumulation noise of a rounding boundary may come out a step off: that step, through |w3| (|w1|), joins the bound
    of what is computed from it.  Split: nothing is rounded in between; the noise of a stage reaches the next through |w| in its scale.
    conv2's weights have a mean of a quarter of their deviation: on zero-mean weights the sums over the (positive, post-ReLU) t1 cancel, s2 / |t2| is
    2 and more, and the share of t2 within A(K2) s2 of a boundary -- about 2 A(K2) / 2^-10.5 x s2 / |t2| of the positive half -- comes to 4.5 - 5.5 % at
    K2 = 1152, where the flags would stop meaning 'few'.  With the mean it is about 3 %, and a tenth of t2 still ends in the ReLU.
    Two more cases (Case.w2_mean = 0) keep the zero-mean draw, whose sums cancel as the engine's do.  Their limit on the share is 10 %: for a sum z s2 with
    z ~ N(0,1) the chance of a boundary within A s2 is min(1, c / |z|) with c = 2 A(K2) / 2^-11 = 0.032 at K2 = 1152 against the smallest ulp of a binade,
    whose mean over z > 0 is (P(|z| < c) + c * 2.8) / 2 = 5.8 % (4 % against the mean ulp); 10 % leaves that estimate a factor of 1.7 and still means 'few'."""
    from proj_roadsurf_amd.weights import _perm_k64, split_planes
    c = case
    rng = _rng("bounds " + c.tag)
    cb, c4, split = c.width, 4 * c.width, c.split
    P = Problem()
    P.case = c
    relu_act = lambda ch: np.maximum(_spread_act(rng, c.n, c.h, c.w, ch), 0)
    P.t1, t1v = _stored(_haloed(relu_act(cb), 1), split)
    P.x, xv = _stored(_haloed(relu_act(64 if c.proj else c4), 1), split)
    xv = xv[:, 1:-1, 1:-1]
    w2, w3, wsc, w1 = _spread_weight(rng, cb, 9 * cb, mean=c.w2_mean), _spread_weight(rng, c4, cb), _spread_weight(rng, c4, 64), _spread_weight(rng, cb, c4)
    P.b2, P.b3, P.b1 = (rng.standard_normal(ch).astype(np.float32) for ch in (cb, c4, cb))
    if split:
        w3k = np.concatenate([_perm_k64(w3, cb), wsc], 1) if c.proj else _perm_k64(w3, cb)
        (P.w2, P.s2), (P.w3, P.s3), (P.w1, P.s1) = (split_planes(m) for m in (w2, w3k, _perm_k64(w1, 64)))
        eff = lambda m: (lambda ws, wsi: (ws[:len(wsi)].astype(np.float64) + ws[len(wsi):].astype(np.float64)) * wsi.astype(np.float64)[:, None])(*split_planes(m))
        w2v, w3v, w1v = eff(w2), eff(w3), eff(w1)
        wscv = eff(np.concatenate([w3, wsc], 1))[:, cb:] if c.proj else None          # the row scale is that of the concatenated row
        if c.proj:
            w3v = eff(np.concatenate([w3, wsc], 1))[:, :cb]
    else:
        h16 = lambda m: m.astype(np.float16)
        P.w2, P.w3, P.w1, P.wsc = h16(w2), _perm_k64(h16(w3), cb), _perm_k64(h16(w1), 64), h16(wsc)
        w2v, w3v, w1v, wscv = (h16(m).astype(np.float64) for m in (w2, w3, w1, wsc))
    b2, b3, b1 = (b.astype(np.float64) for b in (P.b2, P.b3, P.b1))
    p2 = _patches(t1v, 3, 1, 1, 1, c.h, c.w)
    pre2 = p2 @ w2v.T + b2
    s2 = np.sqrt((p2 * p2) @ (w2v * w2v).T) + np.abs(b2)
    short = xv @ wscv.T if c.proj else xv
    s_short = np.sqrt((xv * xv) @ (wscv * wscv).T) if c.proj else np.abs(xv)
    k2, k3, k1 = 9 * cb, cb + (64 if c.proj else 0), c4
    P.K = (k2, k3, k1)
    if split:
        t2 = np.maximum(pre2, 0.0)
        out = np.maximum(t2 @ w3v.T + b3 + short, 0.0)
        t1n = np.maximum(out @ w1v.T + b1, 0.0)
        s3 = np.sqrt((t2 * t2) @ (w3v * w3v).T) + np.sqrt((s2 * s2) @ (w3v * w3v).T) + np.abs(b3) + s_short + 1e-30
        s1 = np.sqrt((out * out) @ (w1v * w1v).T) + np.sqrt((s3 * s3) @ (w1v * w1v).T) + np.abs(b1) + 1e-30
        P.out_ref, P.out_bound = out, (A(k2) + A(k3)) * s3
        P.t1n_ref, P.t1n_bound = t1n, (A(k2) + A(k3) + A(k1)) * s1
        P.flagged = 0.0
    else:
        t2, d2 = _r16_relu_span(pre2, allowance(k2) * s2)
        P.flagged = float((d2 > 0).mean())
        pre3 = t2 @ w3v.T + b3 + short
        s3 = np.sqrt((t2 * t2) @ (w3v * w3v).T) + np.abs(b3) + s_short
        e3 = allowance(k3) * s3 + d2 @ np.abs(w3v).T
        out, d3 = _r16_relu_span(pre3, e3)
        P.out_ref = np.maximum(pre3, 0.0)
        P.out_bound = e3 + 2.0 ** -11 * (P.out_ref + e3) + 2.0 ** -25
        pre1 = out @ w1v.T + b1
        s1 = np.sqrt((out * out) @ (w1v * w1v).T) + np.abs(b1)
        e1 = allowance(k1) * s1 + d3 @ np.abs(w1v).T
        P.t1n_ref = np.maximum(pre1, 0.0)
        P.t1n_bound = e1 + 2.0 ** -11 * (P.t1n_ref + e1) + 2.0 ** -25
    P.planes = 2 if split else 1
    for a in (P.out_ref, P.t1n_ref):
        assert np.all(np.abs(a) < 60000.0), "reference reaches the fp16 clamp"
    assert np.all(np.abs(SENTINEL * P.planes - P.out_ref) > 2.0 * P.out_bound + 1.0) and np.all(np.abs(SENTINEL * P.planes - P.t1n_ref) > 2.0 * P.t1n_bound + 1.0)
    assert P.flagged < c.flag_limit, "%.1f %% of t2 lie within their noise of a rounding boundary" % (100 * P.flagged)
    return P


def check_map(tag, buf, ref, bnd, planes):
    """check_output for a [planes][n][h + 2][w + 2][c] fp16 map with halo 1 that the kernel writes everywhere inside"""
    assert_halo_untouched(buf, 1, tag + ": kernel wrote into the halo")
    got = buf[..., 1:-1, 1:-1, :].astype(np.float64)
    if planes == 2:
        got = got[0] + got[1]
    ratio = np.abs(got - ref.reshape(got.shape)) / bnd.reshape(got.shape)
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = np.unravel_index(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio)), ratio.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %r, ref %r, bound %r (err / bound %.3f)" % (
            tag, int((~(ratio <= 1.0)).sum()), ratio.size, i, got[i], ref.reshape(got.shape)[i], bnd.reshape(got.shape)[i], ratio[i]))
    return worst
