#!/usr/bin/env python3
"""A/B of the training diagnostics: ``set_train_stats(False)`` against ``True`` on one trainer.

    python tools/train_stats_ab.py [--precision fp32] [--rounds 4] [--steps 4] [--warmup 2] [--batch 8] [--out DIR]

One process, ONE trainer at the setting of bench.py --train (batch 8 of 512x512x3 tiles -> 800x800), the switch alternated between
windows of steps (forward, backward, SGD; the table is read once per step when the switch is on, as a run that logs every iteration
would).  After the timing, profiled steps with the switch on give the HIP-event times of the three counting stages next to those of
the loss stages they follow.  Prints one JSON line, writes it to DIR/train_stats_ab.json and the stage table to DIR/stage_table.txt."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("off", "on")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("train_stats_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import Trainer
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    out = {"tool": "tools/train_stats_ab.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "tile": args.tile,
           "batch": args.batch, "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup}
    spec = EngineSpec(num_classes=2, precision=args.precision)
    W = synthetic_weights(spec, seed=0)
    T, B = args.tile, args.batch
    s = 800.0 / T
    tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
    nb = [b * np.float32(s) for b in boxes]
    npoly = [[[p * s for p in inst] for inst in img] for img in polys]
    tr = Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1.0 if args.precision == "fp32" else 1024.0)
    table = []
    try:
        def window(mode, n, seed0):
            tr.set_train_stats(mode == "on")
            tr.sync()
            t0 = time.perf_counter()
            stats = None
            for it in range(n):
                tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                if mode == "on":
                    stats = tr.train_stats()
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / n * 1e3, stats

        for m in MODES:
            window(m, args.warmup, 100)
        ms = {m: [] for m in MODES}
        last = None
        for r in range(args.rounds):
            for m in (MODES if r % 2 == 0 else MODES[::-1]):
                dt, st = window(m, args.steps, 1000 + r * args.steps)
                ms[m].append(dt)
                last = st or last
        for m in MODES:
            out[m] = {"ms_per_step_windows": [round(v, 3) for v in ms[m]], "ms_per_step_median": statistics.median(ms[m]),
                      "ms_per_step_min": min(ms[m]), "ms_per_step_max": max(ms[m])}
        out["scalars_last_step"] = last
        # the stages' own time from the per-stage HIP events (a run of its own: events slow the host)
        tr.set_train_stats(True)
        tr.set_profiling(True)
        window("on", 3, 5000)
        st = {x["name"]: x["ms_total"] / x["calls"] for x in tr.stage_times() if x["calls"]}
        tr.set_profiling(False)
        stats = {k: v for k, v in st.items() if k.endswith(".stats")}
        loss = {k: v for k, v in st.items() if k in ("box.loss", "mask.loss") or k.startswith("rpn.loss")}
        out["stats_stage_ms_per_step"] = {k: round(v, 4) for k, v in stats.items()}
        out["loss_stage_ms_per_step"] = {k: round(v, 4) for k, v in loss.items()}
        out["stats_stages_ms_per_step_sum"] = sum(stats.values())
        out["loss_stages_ms_per_step_sum"] = sum(loss.values())
        table.append("# ms per step from HIP events over 3 profiled steps, switch on")
        for k, v in list(loss.items()) + list(stats.items()):
            table.append(f"{k:16s} {v:9.4f}")
        table.append(f"{'loss stages':16s} {sum(loss.values()):9.4f}")
        table.append(f"{'stats stages':16s} {sum(stats.values()):9.4f}")
        print(f"switch off {out['off']['ms_per_step_median']:.2f} ms/step   on {out['on']['ms_per_step_median']:.2f} ms/step   "
              f"stats stages {sum(stats.values()):.4f} ms   loss stages {sum(loss.values()):.4f} ms", file=sys.stderr, flush=True)
    finally:
        tr.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "train_stats_ab.json"), "w") as f:
            f.write(line + "\n")
        with open(os.path.join(args.out, "stage_table.txt"), "w") as f:
            f.write("\n".join(table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
