#!/usr/bin/env python3
"""A/B of the two input-gradient modes of the fp32 trainer: ``set_dgrad_mode("f32")`` against ``"split"``.

    python tools/dgrad_split_ab.py [--rounds 4] [--steps 4] [--warmup 2] [--batch 8] [--out DIR] [--skip-step] [--skip-ops]

Operator part: four input-gradient shapes of the batch-8 step (the p2 3x3 256 -> 256 map, a res4 1x1 layer, fc1, the 16-row RPN head on
p2), the fp32 matrix-core kernel (rs_op_conv2d, use_glds = -1, on the same dy and w_t) against rs_op_conv2d_dgrad_split with its abs-max,
plane and row-split passes and its allocation included; HIP events around windows of calls, the two interleaved, median of the windows.

Step part: one process, ONE fp32 trainer (the setting of bench.py --train: batch 8 of 512x512x3 tiles -> 800x800), the dgrad mode switched
between windows, once with the weight gradients in mode f32 and once in mode split.  After the timing each mode runs profiled steps and
the per-stage HIP events of the ``*.x`` stages are listed and summed: in split mode they include the abs-max and the plane pass.
Prints one JSON line and writes it to DIR/dgrad_split_ab.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, n, ho, wo, cout (K side), cin (rows), k
OP_SHAPES = [("p2 3x3 256->256", 8, 200, 200, 256, 256, 3), ("res4 conv3 1x1 1024->256", 8, 50, 50, 1024, 256, 1),
             ("fc1 1024->12544", 1, 8192, 1, 1024, 12544, 1), ("rpn head p2 16(64)->256", 8, 200, 200, 64, 256, 1)]


def operators(lib, torch, rounds, calls):
    from proj_roadsurf_amd.engine import _check
    dev = "cuda:0"
    out = []
    for name, n, ho, wo, cout, cin, k in OP_SHAPES:
        h = 1 if wo > 1 else 0
        pad = k // 2
        kpad = k * k * cout
        g = torch.Generator(device=dev).manual_seed(1)
        dy = torch.zeros((n, ho + 2 * h, wo + 2 * h, cout), device=dev)
        dy[:, h:h + ho, h:h + wo] = torch.randn((n, ho, wo, cout), device=dev, generator=g) * 0.1
        w = torch.randn((cin, kpad), device=dev, generator=g) * 0.05
        dx = torch.zeros((n, ho + 2 * h, wo + 2 * h, cin), device=dev)
        bias = torch.zeros(cin + 64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr())

        def f32():
            _check(lib, lib.rs_op_conv2d(p(dy), p(w), p(bias), p(dx), None, None, n, ho, wo, cout, h, k, k, 1, pad, cin, kpad, h, 0, 1, 0, -1, -1, None), "rs_op_conv2d")

        def split():
            _check(lib, lib.rs_op_conv2d_dgrad_split(p(dy), p(w), p(dx), None, None, None, None, n, ho, wo, cin, ho, wo, cout, k, k, 1, pad, kpad, h, -1, None, None),
                   "rs_op_conv2d_dgrad_split")

        ms = {"f32": [], "split": []}
        for fn in (f32, split):
            fn()
        torch.cuda.synchronize()
        for r in range(rounds):
            for key, fn in ((("f32", f32), ("split", split)) if r % 2 == 0 else (("split", split), ("f32", f32))):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[key].append(e0.elapsed_time(e1) / calls)
        flops = 2.0 * n * ho * wo * kpad * cin
        row = {"shape": name, "f32_ms": statistics.median(ms["f32"]), "split_ms": statistics.median(ms["split"]),
               "f32_windows": [round(v, 4) for v in ms["f32"]], "split_windows": [round(v, 4) for v in ms["split"]]}
        row["f32_tflops"], row["split_tflops"] = flops / row["f32_ms"] / 1e9, flops / row["split_ms"] / 1e9
        print(f"{name}: f32 {row['f32_ms']:.3f} ms ({row['f32_tflops']:.0f} TFLOP/s)   split with its passes {row['split_ms']:.3f} ms ({row['split_tflops']:.0f} TFLOP/s)",
              file=sys.stderr, flush=True)
        out.append(row)
        del dy, w, dx
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dgrad_split_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import DGRAD_MODES, Trainer, load_library
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    out = {"tool": "tools/dgrad_split_ab.py", "device": torch.cuda.get_device_name(0), "tile": args.tile, "batch": args.batch,
           "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup}
    if not args.skip_ops:
        out["operators"] = operators(load_library(), torch, max(args.rounds, 5), 5)
    if not args.skip_step:
        spec = EngineSpec(num_classes=2, precision="fp32")
        W = synthetic_weights(spec, seed=0)
        T, B = args.tile, args.batch
        s = 800.0 / T
        tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
        nb = [b * np.float32(s) for b in boxes]
        npoly = [[[p * s for p in inst] for inst in img] for img in polys]
        tr = Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1.0)
        try:
            def window(mode, n, seed0):
                tr.set_dgrad_mode(mode)
                tr.sync()
                t0 = time.perf_counter()
                for it in range(n):
                    l = tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                    tr.apply_sgd(1e-6, 0.9, 1e-4)
                tr.sync()
                return (time.perf_counter() - t0) / n * 1e3, l
            for wgrad in ("f32", "split"):
                tr.set_wgrad_mode(wgrad)
                res = out[f"step_wgrad_{wgrad}"] = {}
                for m in DGRAD_MODES:
                    window(m, args.warmup, 100)
                ms = {m: [] for m in DGRAD_MODES}
                last = {}
                for r in range(args.rounds):
                    for m in (DGRAD_MODES if r % 2 == 0 else DGRAD_MODES[::-1]):
                        dt, last[m] = window(m, args.steps, 1000 + r * args.steps)
                        ms[m].append(dt)
                for m in DGRAD_MODES:
                    res[m] = {"ms_per_step_windows": [round(v, 3) for v in ms[m]], "ms_per_step_median": statistics.median(ms[m]),
                              "ms_per_step_min": min(ms[m]), "ms_per_step_max": max(ms[m]),
                              "losses_last_step": {k: float(v) for k, v in last[m].items()}}
                res["every_split_window_below_every_f32_window"] = max(ms["split"]) < min(ms["f32"])
                # the input-gradient stages' own time from the per-stage HIP events (a run of its own: events slow the host)
                for m in DGRAD_MODES:
                    tr.set_profiling(True)
                    window(m, 3, 5000)
                    xst = {x["name"]: x["ms_total"] / x["calls"] for x in tr.stage_times() if x["calls"] and x["name"].endswith(".x")}
                    tr.set_profiling(False)
                    res[m]["x_stage_ms_per_step"] = {k: round(v, 4) for k, v in sorted(xst.items(), key=lambda kv: -kv[1])}
                    res[m]["x_stages_ms_per_step_sum"] = sum(xst.values())
                print(f"wgrad {wgrad}: dgrad f32 {res['f32']['ms_per_step_median']:.2f} ms/step (*.x stages {res['f32']['x_stages_ms_per_step_sum']:.2f} ms)   "
                      f"dgrad split {res['split']['ms_per_step_median']:.2f} ms/step (*.x stages {res['split']['x_stages_ms_per_step_sum']:.2f} ms)",
                      file=sys.stderr, flush=True)
        finally:
            tr.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "dgrad_split_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
