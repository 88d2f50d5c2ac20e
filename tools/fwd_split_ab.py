#!/usr/bin/env python3
"""A/B of the two forward modes of the fp32 trainer: ``set_fwd_mode("f32")`` against ``"split"``.

    python tools/fwd_split_ab.py [--rounds 4] [--steps 4] [--warmup 2] [--batch 8] [--out DIR]

One process, ONE fp32 trainer (the setting of bench.py --train: batch 8 of 512x512x3 tiles -> 800x800), the fwd mode switched between
windows of steps, once with the weight and input gradients in mode f32 and once with both in mode split.  After the timing each mode
runs profiled steps and the per-stage HIP events of the forward stages (every stage that is not ``bwd.*``) are listed and summed: in split
mode a conv / linear stage includes its abs-max and plane pass.  Before any of it, one step per mode on the same batch and seed without
an SGD step between them gives the relative L2 distance between the modes of p2..p6 and of every gradient tensor.
Prints one JSON line, writes it to DIR/fwd_split_ab.json and the per-stage table to DIR/stage_table.txt."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fwd_split_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import FWD_MODES, Trainer
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    out = {"tool": "tools/fwd_split_ab.py", "device": torch.cuda.get_device_name(0), "tile": args.tile, "batch": args.batch,
           "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup}
    spec = EngineSpec(num_classes=2, precision="fp32")
    W = synthetic_weights(spec, seed=0)
    T, B = args.tile, args.batch
    s = 800.0 / T
    tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
    nb = [b * np.float32(s) for b in boxes]
    npoly = [[[p * s for p in inst] for inst in img] for img in polys]
    tr = Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1.0)
    table = []
    try:
        # ---- distance between the modes: the same batch, seed and weights
        grads = [n for n in tr.tensor_names() if n.startswith("g:")]
        snap = {}
        for m in FWD_MODES:
            tr.set_fwd_mode(m)
            losses = tr.train_step(tiles, nb, classes, npoly, seed=77)
            snap[m] = {"losses": {k: float(v) for k, v in losses.items()}}
            snap[m].update({f"p{l}": tr.tensor(f"p{l}", engine=True).copy() for l in range(2, 7)})
            snap[m].update({n: tr.tensor(n).copy() for n in grads})
        dist = {n: rel_l2(snap["split"][n], snap["f32"][n]) for n in snap["f32"] if n != "losses"}
        out["mode_distance_rel_l2"] = {"p2..p6": {f"p{l}": dist[f"p{l}"] for l in range(2, 7)},
                                       "gradients_worst": dict(sorted(((n, d) for n, d in dist.items() if n.startswith("g:")), key=lambda kv: -kv[1])[:8]),
                                       "gradients_max": max(d for n, d in dist.items() if n.startswith("g:")),
                                       "gradients_median": statistics.median(d for n, d in dist.items() if n.startswith("g:")),
                                       "gradient_tensors": len(grads)}
        out["losses_same_batch"] = {m: snap[m]["losses"] for m in FWD_MODES}
        del snap

        def window(mode, n, seed0):
            tr.set_fwd_mode(mode)
            tr.sync()
            t0 = time.perf_counter()
            for it in range(n):
                l = tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / n * 1e3, l

        for grad in ("f32", "split"):
            tr.set_wgrad_mode(grad)
            tr.set_dgrad_mode(grad)
            res = out[f"step_wgrad_dgrad_{grad}"] = {}
            for m in FWD_MODES:
                window(m, args.warmup, 100)
            ms = {m: [] for m in FWD_MODES}
            last = {}
            for r in range(args.rounds):
                for m in (FWD_MODES if r % 2 == 0 else FWD_MODES[::-1]):
                    dt, last[m] = window(m, args.steps, 1000 + r * args.steps)
                    ms[m].append(dt)
            for m in FWD_MODES:
                res[m] = {"ms_per_step_windows": [round(v, 3) for v in ms[m]], "ms_per_step_median": statistics.median(ms[m]),
                          "ms_per_step_min": min(ms[m]), "ms_per_step_max": max(ms[m]),
                          "losses_last_step": {k: float(v) for k, v in last[m].items()}}
            res["every_split_window_below_every_f32_window"] = max(ms["split"]) < min(ms["f32"])
            # the forward stages' own time from the per-stage HIP events (a run of its own: events slow the host)
            for m in FWD_MODES:
                tr.set_profiling(True)
                window(m, 3, 5000)
                st = {x["name"]: x["ms_total"] / x["calls"] for x in tr.stage_times() if x["calls"] and not x["name"].startswith("bwd.")}
                tr.set_profiling(False)
                res[m]["forward_stage_ms_per_step"] = {k: round(v, 4) for k, v in st.items()}
                res[m]["forward_stages_ms_per_step_sum"] = sum(st.values())
            a, b = res["f32"]["forward_stage_ms_per_step"], res["split"]["forward_stage_ms_per_step"]
            table.append(f"# wgrad / dgrad {grad}: forward stages, ms per step from HIP events over 3 profiled steps (f32, split, split - f32)")
            for k in a:
                table.append(f"{k:28s} {a[k]:9.4f} {b.get(k, float('nan')):9.4f} {b.get(k, float('nan')) - a[k]:+9.4f}")
            table.append(f"{'sum':28s} {sum(a.values()):9.4f} {sum(b.values()):9.4f} {sum(b.values()) - sum(a.values()):+9.4f}")
            res["stages_that_lose"] = sorted(k for k in a if k in b and b[k] > a[k] * 1.05 and b[k] - a[k] > 0.02)
            print(f"wgrad / dgrad {grad}: fwd f32 {res['f32']['ms_per_step_median']:.2f} ms/step (forward stages {res['f32']['forward_stages_ms_per_step_sum']:.2f} ms)   "
                  f"fwd split {res['split']['ms_per_step_median']:.2f} ms/step (forward stages {res['split']['forward_stages_ms_per_step_sum']:.2f} ms)",
                  file=sys.stderr, flush=True)
    finally:
        tr.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "fwd_split_ab.json"), "w") as f:
            f.write(line + "\n")
        with open(os.path.join(args.out, "stage_table.txt"), "w") as f:
            f.write("\n".join(table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
