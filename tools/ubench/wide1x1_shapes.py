#!/usr/bin/env python3
"""Split-operand 1x1 layers with K = 256 and 1024 rows, per batch size: res4.x.conv3 (50 x 50 pixels per tile, residual + ReLU; rs_op_conv2d_split) and the mask
head's fused deconv + predictor (100 entries of 14 x 14 per tile, all of them counted; rs_op_deconv_predict_split, with the logits' memset where the variant
accumulates).  Times conv_wide1x1_split.hip at its three tile heights (variants 29 / 30 / 31 = 64 / 128 / 256 pixels) against the tiles the rule picked
before it.  Kernel time by HIP events on the null stream, 40 back-to-back launches after a warm-up, three rounds in alternating order; one JSON line per
(layer, batch).  Usage: wide1x1_shapes.py [batches, default 1,2,4,8,16]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from proj_roadsurf_amd import engine as E

lib = E.load_library(os.environ.get("RS_LIB") or None)
dev = torch.device("cuda:0")
BATCHES = [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "1,2,4,8,16").split(",")]
P = lambda t: C.c_void_p(t.data_ptr())


def timed(call, reps=40):
    for _ in range(5):
        assert call() == 0, lib.rs_last_error()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # us


def sweep(name, batch, variants, make_call):
    best = {v: [] for v in variants}
    for rnd in range(3):
        for v in (variants if rnd % 2 == 0 else variants[::-1]):
            best[v].append(round(timed(make_call(v)), 1))
    print(json.dumps({"layer": name, "batch": batch, "us": {str(v): best[v] for v in variants}}), flush=True)


for B in BATCHES:
    # res4.x.conv3
    n, h = B, 50
    x = (torch.randn((2, n, h + 2, h + 2, 256), device=dev) * 0.5).half()
    wt = (torch.randn((2, 1024, 256), device=dev) * 100.0).half()
    sc = torch.full((1024,), 1e-4, dtype=torch.float32, device=dev)
    b = torch.zeros(1024, dtype=torch.float32, device=dev)
    out = torch.zeros((2, n, h + 2, h + 2, 1024), dtype=torch.float16, device=dev)
    r = torch.randn((2, n, h + 2, h + 2, 1024), device=dev).half()

    def conv_call(v):
        return lambda: lib.rs_op_conv2d_split(P(x), x[0].numel(), P(wt), wt[0].numel(), P(sc), P(b), P(out), out[0].numel(), P(r), r[0].numel(), None, 0,
                                              n, h, h, 256, 1, 1, 1, 1, 0, 1024, 256, 1, 1, 0, 0, v, None)
    sweep("res4.x.conv3", B, [12, 15, 7, 0, 14, 29, 30, 31], conv_call)

    # mask.deconv_predict
    ent, side = 100 * B, 14
    xm = (torch.randn((2, ent, side + 2, side + 2, 256), device=dev).abs() * 0.5).half()
    dw = torch.randn((2, 256), device=dev)
    cls = torch.randint(0, 2, (ent,), dtype=torch.int32, device=dev)
    slot = torch.randperm(ent, device=dev).int()
    cnt = torch.tensor([ent], dtype=torch.int32, device=dev)
    logits = torch.zeros((ent, 2 * side, 2 * side), dtype=torch.float32, device=dev)

    def mask_call(v):
        def f():
            if v < 28:
                logits.zero_()
            return lib.rs_op_deconv_predict_split(P(xm), xm[0].numel(), P(wt), wt[0].numel(), P(sc), P(b), P(dw), 2, P(cls), P(slot), P(cnt), P(logits),
                                                  ent, side, v, None)
        return f
    sweep("mask.deconv_predict", B, [14, 10, 29, 30, 31], mask_call)
