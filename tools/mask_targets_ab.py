#!/usr/bin/env python3
"""A/B of the two mask-target paths of the training step: ``Trainer(mask_targets="host")`` against ``"device"``.

    python tools/mask_targets_ab.py [--rounds 6] [--steps 10] [--warmup 4] [--out DIR]

One process, one trainer per mode on the same weights.  Per case both trainers first run the warm-up steps (every kernel and shape of
the timed window), then ``rounds`` windows of ``steps`` x (train_step + apply_sgd) are timed alternately -- host, device, host, ... --
each closed by a device synchronise; the same batches and seeds go to both, and the losses of the last step are compared.  Cases:
the benchmark's tile shape (512x512x3 -> 800x800, fp16) at batch 8 and batch 1 with the ground truth of synthetic.synthetic_scenes
(bench.py --train's workload), and batch 8 once more with every instance outlined by a few hundred vertices.  After the timing the
device trainer runs a few profiled steps for the kernel's own time (stage "mask.targets") and the host trainer for the stages of
the path it replaces.  Prints one JSON line and writes it to DIR/mask_targets_ab.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def densify(poly: np.ndarray, vertices: int) -> np.ndarray:
    """The same outline with `vertices` vertices spread evenly over its edges."""
    p = poly.reshape(-1, 2)
    k = len(p)
    per = max(1, vertices // k)
    t = np.arange(per)[:, None] / per
    return np.concatenate([p[i] + t * (p[(i + 1) % k] - p[i]) for i in range(k)]).reshape(-1)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--vertices", type=int, default=400, help="vertices per instance in the long-polygon case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mask_targets_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import Trainer
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    T = args.tile
    s = 800.0 / T
    out = {"tool": "tools/mask_targets_ab.py", "device": torch.cuda.get_device_name(0), "tile": T, "precision": spec.precision,
           "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup, "cases": []}
    for name, B, vertices in (("batch8", 8, 0), ("batch1", 1, 0), ("batch8_long_polygons", 8, args.vertices)):
        tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
        nb = [b * np.float32(s) for b in boxes]
        npoly = [[[(densify(p, vertices) if vertices else p) * s for p in inst] for inst in img] for img in polys]
        tr = {m: Trainer(spec, W, (T, T, 3), batch=B, loss_scale=1024.0, mask_targets=m) for m in ("host", "device")}
        try:
            def window(m, n, seed0):
                t0 = time.perf_counter()
                for it in range(n):
                    l = tr[m].train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                    tr[m].apply_sgd(1e-5, 0.9, 1e-4)
                tr[m].sync()
                return (time.perf_counter() - t0) / n * 1e3, l
            for m in tr:
                window(m, args.warmup, 100)
            ms = {m: [] for m in tr}
            last = {}
            for r in range(args.rounds):
                for m in (("host", "device") if r % 2 == 0 else ("device", "host")):
                    dt, last[m] = window(m, args.steps, 1000 + r * args.steps)
                    ms[m].append(dt)
            rec = {"case": name, "batch": B, "vertices_per_instance": vertices or "synthetic_scenes (4 or 24)",
                   "instances": int(sum(len(img) for img in npoly)), "mask_entries_last_step": int(tr["device"].tensor("mask_total")[0]),
                   "losses_identical_last_step": last["host"] == last["device"], "fallbacks": tr["device"].mask_target_fallbacks}
            for m in tr:
                rec[f"{m}_ms_per_step_windows"] = [round(v, 4) for v in ms[m]]
                rec[f"{m}_ms_per_step_median"] = statistics.median(ms[m])
                rec[f"{m}_ms_per_step_min"] = min(ms[m])
            rec["device_minus_host_ms_median"] = rec["device_ms_per_step_median"] - rec["host_ms_per_step_median"]
            # the kernel's own time, and the stages around it, from the per-stage HIP events (a run of its own: events slow the host)
            for m in tr:
                tr[m].set_profiling(True)
                window(m, 4, 5000)
                st = {x["name"]: x for x in tr[m].stage_times() if x["calls"]}
                tr[m].set_profiling(False)
                rec[f"{m}_stage_ms_per_step"] = {k: st[k]["ms_total"] / st[k]["calls"] for k in ("mask.targets", "mask.entries", "mask.loss") if k in st}
            out["cases"].append(rec)
            print(f"[{name}] host {rec['host_ms_per_step_median']:.3f} ms  device {rec['device_ms_per_step_median']:.3f} ms  "
                  f"mask.targets {rec['device_stage_ms_per_step'].get('mask.targets', float('nan')):.4f} ms", file=sys.stderr, flush=True)
        finally:
            for t in tr.values():
                t.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "mask_targets_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
