#!/usr/bin/env python3
"""Step and stage times of the trainer at MODEL.BACKBONE.FREEZE_AT 2, 1 and 0.

    python tools/freeze_at_stages.py [--precision fp32] [--rounds 3] [--steps 4] [--warmup 2] [--batch 8] [--out DIR]

One process, one trainer per value at the setting of bench.py --train (batch 8 of 512x512x3 tiles -> 800x800).  The step (forward,
backward, SGD) is timed in windows that alternate between the three trainers; then profiled steps give the HIP-event time of every
stage, from which the tool reports the stages a value adds, the forward stages of the stem and res2 (the cost of running them unfused),
and for the two stem stages the achieved bytes/s against their algorithmic traffic.  Prints one JSON line, writes it to
DIR/freeze_at_stages.json and the tables to DIR/stage_table.txt."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALUES = (2, 1, 0)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth the fractions are quoted against (MI355X: 8 TB/s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("freeze_at_stages.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import Trainer
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    out = {"tool": "tools/freeze_at_stages.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "tile": args.tile,
           "batch": args.batch, "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup, "hbm_gbs": args.hbm_gbs}
    spec = EngineSpec(num_classes=2, precision=args.precision)
    W = synthetic_weights(spec, seed=0)
    T, B = args.tile, args.batch
    s = 800.0 / T
    tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
    nb = [b * np.float32(s) for b in boxes]
    npoly = [[[p * s for p in inst] for inst in img] for img in polys]
    trs = {fa: Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1.0 if args.precision == "fp32" else 1024.0, freeze_at=fa) for fa in VALUES}
    table = []
    try:
        def window(fa, n, seed0):
            tr = trs[fa]
            tr.sync()
            t0 = time.perf_counter()
            for it in range(n):
                tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / n * 1e3

        for fa in VALUES:
            window(fa, args.warmup, 100)
        ms = {fa: [] for fa in VALUES}
        for r in range(args.rounds):
            for fa in (VALUES if r % 2 == 0 else VALUES[::-1]):
                ms[fa].append(window(fa, args.steps, 1000 + r * args.steps))
        out["step"] = {str(fa): {"ms_per_step_windows": [round(v, 3) for v in ms[fa]], "ms_per_step_median": statistics.median(ms[fa]),
                                 "ms_per_step_min": min(ms[fa]), "ms_per_step_max": max(ms[fa])} for fa in VALUES}
        stages = {}
        for fa in VALUES:
            trs[fa].set_profiling(True)
            window(fa, 3, 5000)
            stages[fa] = {x["name"]: x["ms_total"] / x["calls"] for x in trs[fa].stage_times() if x["calls"]}
            trs[fa].set_profiling(False)
    finally:
        for tr in trs.values():
            tr.close()

    def below_res3(name):
        n = name[4:] if name.startswith("bwd.") else name
        return n.startswith("stem") or n.startswith("res2.")
    out["stages_ms_per_step"] = {}
    for fa in VALUES:
        fwd = {k: v for k, v in stages[fa].items() if below_res3(k) and not k.startswith("bwd.")}
        new = {k: v for k, v in stages[fa].items() if k not in stages[2]} if fa != 2 else {}
        bwd_new = {k: v for k, v in new.items() if k.startswith("bwd.")}
        out["stages_ms_per_step"][str(fa)] = {"forward_stem_and_res2": {k: round(v, 4) for k, v in fwd.items()}, "forward_stem_and_res2_sum": sum(fwd.values()),
                                              "backward_added": {k: round(v, 4) for k, v in bwd_new.items()}, "backward_added_sum": sum(bwd_new.values()),
                                              "all_stages_sum": sum(stages[fa].values())}
        table.append(f"# FREEZE_AT {fa}: ms per step from HIP events over 3 profiled steps ({args.precision} trainer, batch {B})")
        table.append("## forward, stem and res2")
        table += [f"{k:36s} {v:9.4f}" for k, v in fwd.items()] + [f"{'sum':36s} {sum(fwd.values()):9.4f}"]
        if bwd_new:
            table.append("## backward stages this value adds")
            table += [f"{k:36s} {v:9.4f}" for k, v in bwd_new.items()] + [f"{'sum':36s} {sum(bwd_new.values()):9.4f}"]
        table.append(f"{'every stage of the step, summed':36s} {sum(stages[fa].values()):9.4f}")
        table.append("")
    # algorithmic traffic of the two stem stages (at the 800 x 800 network input: stem_conv 400 x 400 x 64, stem 200 x 200 x 64, x0 800 x 800 x 4)
    from proj_roadsurf_amd.spec import resize_shortest_edge_shape
    es = 4 if args.precision == "fp32" else 2
    net_h, _ = resize_shortest_edge_shape(T, T, spec.min_size_test, spec.max_size_test)
    hc = (net_h + spec.size_divisibility - 1) // spec.size_divisibility * spec.size_divisibility // 2      # square tiles: one size
    pool_bytes = B * es * 64 * (2 * hc * hc + (hc // 2) ** 2)            # stem_conv once + d_stem_conv once + d_pool once
    wgrad_bytes = B * es * (hc * hc * 64 + (2 * hc) ** 2 * 4)            # dy once + x0 once
    traffic = {}
    for name, nbytes in (("bwd.stem.maxpool", pool_bytes), ("bwd.stem.conv1.w", wgrad_bytes)):
        t = stages[0].get(name)
        if t:
            gbs = nbytes / (t * 1e-3) / 1e9
            traffic[name] = {"ms": round(t, 4), "algorithmic_bytes": nbytes, "gb_per_s": round(gbs, 1), "fraction_of_hbm": round(gbs / args.hbm_gbs, 4)}
            table.append(f"{name:20s} {t:8.4f} ms  {nbytes / 1e6:9.1f} MB algorithmic  {gbs:8.1f} GB/s  {gbs / args.hbm_gbs:6.3f} of {args.hbm_gbs:.0f} GB/s")
    out["stem_stage_traffic"] = traffic
    wflop = 2.0 * B * hc * hc * 64 * 49 * 3
    if "bwd.stem.conv1.w" in traffic:
        traffic["bwd.stem.conv1.w"]["algorithmic_tflops"] = round(wflop / (traffic["bwd.stem.conv1.w"]["ms"] * 1e-3) / 1e12, 2)
    print("  ".join(f"FREEZE_AT {fa}: {out['step'][str(fa)]['ms_per_step_median']:.2f} ms/step" for fa in VALUES), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "freeze_at_stages.json"), "w") as f:
            f.write(line + "\n")
        with open(os.path.join(args.out, "stage_table.txt"), "w") as f:
            f.write("\n".join(table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
