#!/usr/bin/env python3
"""Output bits of the convolution operators (rs_op_conv2d, rs_op_conv2d_split, rs_op_conv2d_dual, rs_op_conv2d_dgrad,
rs_op_deconv_predict_split, rs_op_bneck_tail, rs_op_bneck_tail_split) on small seeded inputs, every admissible tile variant forced by
number: one sha256 per case.  Two runs with two builds of the library (RS_ENGINE_LIB) are compared case for case; a change of
csrc/conv_tile.h or of a kernel that is meant to keep behaviour must leave every hash as it was.

    conv_op_compare.py --out ops.json            (RS_ENGINE_LIB selects the build)
    conv_op_compare.py --compare A.json B.json

Shapes are the smallest at which the shared pieces can go wrong: one image of 13 x 11 (143 pixels: a ragged last tile for every tile
height, fewer than eight tiles) and two of 24 x 20 (960 pixels: a tile count that is no multiple of eight for the 64- and 128-pixel
tiles).  The fused stems and the fp16 mode-2 predictor have no operator entry; tools/parity/engine_manifest.py covers them."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.conv_cases import WIDE, _variants, IGEMM, tool_cases      # noqa: E402  (the case grid, shared with tests/test_gpu_conv_bounds.py)
from tests.conv_cases import bneck_tag, conv_tag, deconv_predict_tag, dgrad_tag, dual_tag      # noqa: E402


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _act(rng, n, h, w, c, halo, scale=1.0):
    """[n][h + 2 halo][w + 2 halo][c] fp32 with a zero halo"""
    a = np.zeros((n, h + 2 * halo, w + 2 * halo, c), np.float32)
    a[:, halo:halo + h, halo:halo + w] = rng.standard_normal((n, h, w, c)).astype(np.float32) * scale
    return a


def _planes(a32):
    hi = a32.astype(np.float16)
    return np.stack([hi, (a32 - hi.astype(np.float32)).astype(np.float16)])


class Runner:
    def __init__(self):
        import torch
        from proj_roadsurf_amd.engine import load_library
        from proj_roadsurf_amd.weights import split_planes
        self.torch, self.lib, self.split_planes = torch, load_library(), split_planes
        self.dev = torch.device("cuda:0")
        self.out = {}

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def zeros(self, shape, dtype):
        return self.torch.zeros(shape, dtype=dtype, device=self.dev)

    @staticmethod
    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def record(self, name, rc, *tensors):
        self.torch.cuda.synchronize()
        if rc != 0:
            self.out[name] = "refused: rc %d" % rc
            return
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.cpu().numpy().tobytes())
        self.out[name] = h.hexdigest()

    # ---- rs_op_conv2d / rs_op_conv2d_split
    def conv(self, split, n, h, w, cin, cout, k, stride, res, up, relu, deconv=False, out_f32=False):
        T = self.torch
        pad = k // 2
        tag = conv_tag(split, n, h, w, cin, cout, k, stride, res, up, relu, deconv, out_f32)
        rng = _rng(tag)
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        oh, ow = (2 * ho, 2 * wo) if deconv else (ho, wo)
        rows = cout * (4 if deconv else 1)
        x32 = _act(rng, n, h, w, cin, pad)
        w32 = rng.standard_normal((rows, k * k * cin)).astype(np.float32) * np.float32(0.05)
        bias = self.up(rng.standard_normal(rows).astype(np.float32))
        r32 = _act(rng, n, oh, ow, cout, 1) if res else None
        u32 = _act(rng, n, ho // 2, wo // 2, cout, 1) if up else None
        oshape = (n, oh + 2, ow + 2, cout)
        if split:
            ws, wsi = self.split_planes(w32)
            xd, wd, sd = self.up(_planes(x32)), self.up(ws), self.up(wsi)
            rd = self.up(_planes(r32)) if res else None
            ud = self.up(_planes(u32)) if up else None
        else:
            xd, wd = self.up(x32.astype(np.float16)), self.up(w32.astype(np.float16))
            rd = self.up(r32.astype(np.float16)) if res else None
            ud = self.up(u32.astype(np.float16)) if up else None
        variants = [-1, 2] if out_f32 else _variants(split, cin, cout, k, stride, res, up, deconv)
        for v in variants:
            if out_f32:
                od = self.zeros(oshape, T.float32)
            else:
                od = self.zeros(((2,) + oshape) if split else oshape, T.float16)
            if split:
                rc = self.lib.rs_op_conv2d_split(self.p(xd), C.c_int64(xd[0].numel()), self.p(wd), C.c_int64(rows * w32.shape[1]), self.p(sd), self.p(bias), self.p(od),
                                                 C.c_int64(0 if out_f32 else od[0].numel()), self.p(rd), C.c_int64(rd[0].numel() if res else 0), self.p(ud),
                                                 C.c_int64(ud[0].numel() if up else 0), n, h, w, cin, pad, k, k, stride, pad, cout, w32.shape[1], 1, int(relu),
                                                 int(out_f32), int(deconv), v, None)
            else:
                rc = self.lib.rs_op_conv2d(self.p(xd), self.p(wd), self.p(bias), self.p(od), self.p(rd), self.p(ud), n, h, w, cin, pad, k, k, stride, pad, cout,
                                           w32.shape[1], 1, int(relu), int(out_f32), int(deconv), v, 1, None)
            self.record("%s v%d" % (tag, v), rc, od)

    # ---- conv3 + projection shortcut over two K sources (fp16)
    def dual(self, n, h, w, cin, cin2, cout, stride2):
        tag = dual_tag(n, h, w, cin, cin2, cout, stride2)
        rng = _rng(tag)
        xd = self.up(_act(rng, n, h, w, cin, 0).astype(np.float16))
        x2 = self.up(_act(rng, n, h * stride2, w * stride2, cin2, 1).astype(np.float16))
        wd = self.up((rng.standard_normal((cout, cin + cin2)) * 0.05).astype(np.float16))
        bias = self.up(rng.standard_normal(cout).astype(np.float32))
        for v in [-1] + [v for v, mult in IGEMM.items() if cout % mult == 0]:
            od = self.zeros((n, h + 2, w + 2, cout), self.torch.float16)
            rc = self.lib.rs_op_conv2d_dual(self.p(xd), self.p(x2), self.p(wd), self.p(bias), self.p(od), n, h, w, cin, 0, 1, 1, 1, 0, h * stride2, w * stride2, cin2, 1,
                                            stride2, cout, cin + cin2, 1, 1, v, None)
            self.record("%s v%d" % (tag, v), rc, od)

    # ---- training epilogues: down / res32 / mask / out_stride through the input-gradient operator
    def dgrad(self, n, hi, wi, cin, cout, k, stride, res, res32, mask, down):
        T = self.torch
        tag = dgrad_tag(n, hi, wi, cin, cout, k, stride, res, res32, mask, down)
        rng = _rng(tag)
        pad = k // 2
        ho, wo = (hi, wi) if stride == 1 else ((hi + stride - 1) // stride, (wi + stride - 1) // stride)
        dy = self.up(_act(rng, n, ho, wo, cout, 1).astype(np.float16))
        wt = self.up((rng.standard_normal((cin, k * k * cout)) * 0.05).astype(np.float16))
        rd = self.up(_act(rng, n, hi, wi, cin, 1).astype(np.float16)) if res else None
        r32 = self.up(_act(rng, n, hi, wi, cin, 1)) if res32 else None
        md = self.up(_act(rng, n, hi, wi, cin, 1).astype(np.float16)) if mask else None
        dn = self.up(_act(rng, n, 2 * hi, 2 * wi, cin, 1).astype(np.float16)) if down else None
        for v in _variants(False, cout, cin, k, 1, False, False, False, train=True, scatter=stride > 1):
            dx = self.zeros((n, hi + 2, wi + 2, cin), T.float16)
            rc = self.lib.rs_op_conv2d_dgrad(self.p(dy), self.p(wt), self.p(dx), self.p(rd), self.p(r32), self.p(md), self.p(dn), n, hi, wi, cin, ho, wo, cout, k, k, stride,
                                             pad, k * k * cout, 1, v, None)
            self.record("%s v%d" % (tag, v), rc, dx)

    # ---- mode 2 in the split mode: fused deconv + predictor, rows bounded by a device count below the capacity
    def deconv_predict(self, entries, count, side):
        T = self.torch
        tag = deconv_predict_tag(entries, count, side)
        rng = _rng(tag)
        classes, slots = 3, entries + 2
        xd = self.up(_planes(np.abs(_act(rng, entries, side, side, 256, 1))))
        ws, wsi = self.split_planes(rng.standard_normal((1024, 256)).astype(np.float32) * np.float32(0.05))
        wd, sd = self.up(ws), self.up(wsi)
        bias, dw = self.up(rng.standard_normal(1024).astype(np.float32)), self.up(rng.standard_normal((classes, 256)).astype(np.float32))
        slot = self.up(rng.permutation(slots)[:entries].astype(np.int32))
        cls = self.up(rng.integers(0, classes, slots).astype(np.int32))
        cnt = self.up(np.array([count], np.int32))
        for v in [-1, 0, 10, 14] + WIDE:
            lg = self.zeros((slots, 2 * side, 2 * side), T.float32)
            rc = self.lib.rs_op_deconv_predict_split(self.p(xd), C.c_int64(xd[0].numel()), self.p(wd), C.c_int64(1024 * 256), self.p(sd), self.p(bias), self.p(dw), classes,
                                                     self.p(cls), self.p(slot), self.p(cnt), self.p(lg), entries, side, v, None)
            self.record("%s v%d" % (tag, v), rc, lg)

    # ---- both bottleneck tails: CB 1 and 2, with / without the next conv1 and the projection shortcut
    def bneck(self, split, n, h, w, width, nxt, proj):
        T = self.torch
        tag = bneck_tag(split, n, h, w, width, nxt, proj)
        rng = _rng(tag)
        c4 = 4 * width
        t1 = _act(rng, n, h, w, width, 1)
        x = _act(rng, n, h, w, c4, 1)
        x0 = _act(rng, n, h, w, 64, 1)
        w2 = rng.standard_normal((width, 9 * width)).astype(np.float32) * np.float32(0.05)
        w3 = rng.standard_normal((c4, width + (64 if (proj and split) else 0))).astype(np.float32) * np.float32(0.05)
        wsc = rng.standard_normal((c4, 64)).astype(np.float32) * np.float32(0.05)
        w1 = rng.standard_normal((width, c4)).astype(np.float32) * np.float32(0.05)
        b2, b3, b1 = (self.up(rng.standard_normal(c).astype(np.float32)) for c in (width, c4, width))
        if split:
            (w2p, s2), (w3p, s3), (w1p, s1) = ((self.up(a), self.up(b)) for a, b in (self.split_planes(m) for m in (w2, w3, w1)))
            t1d, xd, x0d = self.up(_planes(t1)), self.up(_planes(x)), self.up(_planes(x0))
            out, t1n = self.zeros((2, n, h + 2, w + 2, c4), T.float16), self.zeros((2, n, h + 2, w + 2, width), T.float16)
            rc = self.lib.rs_op_bneck_tail_split(self.p(t1d), C.c_int64(t1d[0].numel()), self.p(w2p), self.p(s2), self.p(b2), self.p(w3p), self.p(s3), self.p(b3),
                                                 None if proj else self.p(xd), C.c_int64(xd[0].numel()), self.p(out), C.c_int64(out[0].numel()),
                                                 self.p(w1p) if nxt else None, self.p(s1) if nxt else None, self.p(b1) if nxt else None, self.p(t1n) if nxt else None,
                                                 C.c_int64(t1n[0].numel()), self.p(x0d) if proj else None, C.c_int64(x0d[0].numel()), n, h, w, width, None)
        else:
            h16 = lambda a: self.up(a.astype(np.float16))
            out, t1n = self.zeros((n, h + 2, w + 2, c4), T.float16), self.zeros((n, h + 2, w + 2, width), T.float16)
            rc = self.lib.rs_op_bneck_tail(self.p(h16(t1)), self.p(h16(w2)), self.p(b2), self.p(h16(w3)), self.p(b3), None if proj else self.p(h16(x)), self.p(out),
                                           self.p(h16(w1)) if nxt else None, self.p(b1) if nxt else None, self.p(t1n) if nxt else None,
                                           self.p(h16(x0)) if proj else None, self.p(h16(wsc)) if proj else None, n, h, w, width, None)
        self.record(tag, rc, out, t1n)


def run_all(r):
    for method, args, kw in tool_cases():
        getattr(r, method)(*args, **kw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args(argv)
    if a.compare:
        A, B = (json.load(open(f)) for f in a.compare)
        diff = sorted(k for k in set(A["cases"]) | set(B["cases"]) if A["cases"].get(k) != B["cases"].get(k))
        ran = sum(1 for v in A["cases"].values() if not v.startswith("refused"))
        print("%d cases (%d ran, %d refused by the library), %d differ" % (len(A["cases"]), ran, len(A["cases"]) - ran, len(diff)))
        for k in diff:
            print("DIFF", k, A["cases"].get(k), B["cases"].get(k))
        return 1 if diff else 0
    r = Runner()
    run_all(r)
    json.dump({"lib": os.environ.get("RS_ENGINE_LIB", "in-tree"), "cases": r.out}, open(a.out, "w"), indent=0, sort_keys=True)
    print("%d cases -> %s" % (len(r.out), a.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
