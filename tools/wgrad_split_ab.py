#!/usr/bin/env python3
"""A/B of the two weight-gradient modes of the fp32 trainer: ``set_wgrad_mode("f32")`` against ``"split"``.

    python tools/wgrad_split_ab.py [--rounds 6] [--steps 5] [--warmup 3] [--batch 8] [--out DIR]

One process, ONE fp32 trainer (the setting of bench.py --train: batch 8 of 512x512x3 tiles -> 800x800, the scenes of
synthetic.synthetic_scenes), the mode switched between windows.  Both modes first run the warm-up steps, then ``rounds`` windows of
``steps`` x (train_step + apply_sgd) are timed alternately -- f32, split, f32, ... -- each closed by a device synchronise.  After the
timing each mode runs a few profiled steps and the per-stage HIP events of the ``*.w`` stages are summed: in split mode they include the
abs-max and the plane pass of every layer.  Prints one JSON line and writes it to DIR/wgrad_split_ab.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wgrad_split_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import Trainer, WGRAD_MODES
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2, precision="fp32")
    W = synthetic_weights(spec, seed=0)
    T, B = args.tile, args.batch
    s = 800.0 / T
    tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
    nb = [b * np.float32(s) for b in boxes]
    npoly = [[[p * s for p in inst] for inst in img] for img in polys]
    out = {"tool": "tools/wgrad_split_ab.py", "device": torch.cuda.get_device_name(0), "tile": T, "batch": B, "precision": spec.precision,
           "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup}
    tr = Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1.0)
    try:
        def window(mode, n, seed0):
            tr.set_wgrad_mode(mode)
            tr.sync()
            t0 = time.perf_counter()
            for it in range(n):
                l = tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / n * 1e3, l
        for m in WGRAD_MODES:
            window(m, args.warmup, 100)
        ms = {m: [] for m in WGRAD_MODES}
        last = {}
        for r in range(args.rounds):
            for m in (WGRAD_MODES if r % 2 == 0 else WGRAD_MODES[::-1]):
                dt, last[m] = window(m, args.steps, 1000 + r * args.steps)
                ms[m].append(dt)
        for m in WGRAD_MODES:
            out[m] = {"ms_per_step_windows": [round(v, 3) for v in ms[m]], "ms_per_step_median": statistics.median(ms[m]),
                      "ms_per_step_min": min(ms[m]), "ms_per_step_max": max(ms[m]), "images_per_s_median": B / statistics.median(ms[m]) * 1e3,
                      "losses_last_step": {k: float(v) for k, v in last[m].items()}}
        out["speedup_median"] = out["f32"]["ms_per_step_median"] / out["split"]["ms_per_step_median"]
        # the weight-gradient stages' own time from the per-stage HIP events (a run of its own: events slow the host); switching the
        # profile on clears the totals, so each mode reads its own
        for m in WGRAD_MODES:
            tr.set_profiling(True)
            window(m, 3, 5000)
            wst = {x["name"]: x["ms_total"] / x["calls"] for x in tr.stage_times() if x["calls"] and x["name"].endswith(".w")}
            tr.set_profiling(False)
            out[m]["w_stage_ms_per_step"] = {k: round(v, 4) for k, v in sorted(wst.items(), key=lambda kv: -kv[1])}
            out[m]["w_stages_ms_per_step_sum"] = sum(wst.values())
        print(f"f32 {out['f32']['ms_per_step_median']:.2f} ms/step ({out['f32']['images_per_s_median']:.1f} img/s, *.w stages "
              f"{out['f32']['w_stages_ms_per_step_sum']:.2f} ms)   split {out['split']['ms_per_step_median']:.2f} ms/step "
              f"({out['split']['images_per_s_median']:.1f} img/s, *.w stages {out['split']['w_stages_ms_per_step_sum']:.2f} ms)", file=sys.stderr, flush=True)
    finally:
        tr.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "wgrad_split_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
