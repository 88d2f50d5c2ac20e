#!/usr/bin/env python3
"""A/B of the optimiser step: a trainer whose solver was never set against ``set_solver`` with norm, value and full_model clipping,
and, with ``--parent-lib``, against a trainer on another build of the library (the parent commit's) in the same process.

    python tools/solver_ab.py [--precision fp32] [--rounds 4] [--steps 4] [--warmup 2] [--batch 8] [--parent-lib PATH] [--out DIR]

The setting of bench.py --train (batch 8 of 512x512x3 tiles -> 800x800).  Windows of whole steps (forward, backward, apply_sgd)
alternate between the arms; a solver mode is switched on ONE trainer, the unset arm and the parent arm have trainers of their own (a
solver cannot be unset).  Then, per arm, the optimiser step alone: ``apply_sgd`` calls on the gradient as it stands between two stream
synchronisations (the SGD launches plus the refold of the fp16 operands that every arm shares).  Prints one JSON line and writes it to
DIR/solver_ab_<precision>.json."""
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
    ap.add_argument("--precision", choices=("fp32", "fp16"), default="fp32")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--sgd-calls", type=int, default=20, help="apply_sgd calls per timing of the optimiser step alone")
    ap.add_argument("--parent-lib", default=None, help="librs_engine.so of the parent commit: one more arm, solver unset")
    ap.add_argument("--parent-first", action="store_true", help="create the parent's trainer before the two of this build (the order of creation "
                                                                "decides where a trainer's buffers lie)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("solver_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.engine import SolverOptions, Trainer
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    out = {"tool": "tools/solver_ab.py", "device": torch.cuda.get_device_name(0), "precision": args.precision, "tile": args.tile,
           "batch": args.batch, "rounds": args.rounds, "steps_per_window": args.steps, "warmup_steps": args.warmup, "sgd_calls": args.sgd_calls}
    spec = EngineSpec(num_classes=2, precision=args.precision)
    W = synthetic_weights(spec, seed=0)
    T, B = args.tile, args.batch
    s = 800.0 / T
    tiles, boxes, classes, polys = synthetic_scenes(B, T, T, 3, seed=4321)
    nb = [b * np.float32(s) for b in boxes]
    npoly = [[[p * s for p in inst] for inst in img] for img in polys]
    scale = 1.0 if args.precision == "fp32" else 1024.0
    solvers = {"norm": SolverOptions(clip_type="norm", clip_value=1.0), "value": SolverOptions(clip_type="value", clip_value=1.0),
               "full_model": SolverOptions(clip_type="full_model", clip_value=1.0)}
    trainers = {}
    order = ["unset", "set"] + (["parent"] if args.parent_lib else [])
    for name in (order[::-1] if args.parent_first else order):
        trainers[name] = Trainer(spec, W, (T, T, 3), batch=B, loss_scale=scale, lib_path=args.parent_lib if name == "parent" else None)
    out["created_in_order"] = list(trainers)
    arms = (["parent"] if args.parent_lib else []) + ["unset"] + list(solvers)
    try:
        def trainer_of(arm):
            if arm in solvers:
                trainers["set"].set_solver(solvers[arm])
                return trainers["set"]
            return trainers[arm]

        def window(arm, n, seed0):
            tr = trainer_of(arm)
            tr.sync()
            t0 = time.perf_counter()
            for it in range(n):
                tr.train_step(tiles, nb, classes, npoly, seed=seed0 + it)
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / n * 1e3

        def sgd_alone(arm):
            tr = trainer_of(arm)
            tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            t0 = time.perf_counter()
            for _ in range(args.sgd_calls):
                tr.apply_sgd(1e-6, 0.9, 1e-4)
            tr.sync()
            return (time.perf_counter() - t0) / args.sgd_calls * 1e3

        for a in arms:
            window(a, args.warmup, 100)
        ms = {a: [] for a in arms}
        sgd = {a: [] for a in arms}
        for r in range(args.rounds):
            for a in (arms if r % 2 == 0 else arms[::-1]):
                ms[a].append(window(a, args.steps, 1000 + r * args.steps))
            for a in (arms if r % 2 == 0 else arms[::-1]):
                sgd[a].append(sgd_alone(a))
        for a in arms:
            out[a] = {"ms_per_step_windows": [round(v, 3) for v in ms[a]], "ms_per_step_median": statistics.median(ms[a]),
                      "ms_per_step_min": min(ms[a]), "ms_per_step_max": max(ms[a]),
                      "apply_sgd_ms_windows": [round(v, 4) for v in sgd[a]], "apply_sgd_ms_median": statistics.median(sgd[a])}
        out["grad_norms_minmax"] = [min(trainer_of("norm").grad_norms().values()), max(trainers["set"].grad_norms().values())]
        out["param_count"] = trainers["unset"].param_count
        print("   ".join(f"{a} {out[a]['ms_per_step_median']:.2f} ms/step, apply_sgd {out[a]['apply_sgd_ms_median']:.3f} ms" for a in arms),
              file=sys.stderr, flush=True)
    finally:
        for t in trainers.values():
            t.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"solver_ab_{args.precision}{'_parent_first' if args.parent_first else ''}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
