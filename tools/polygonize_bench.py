#!/usr/bin/env python3
"""What the device polygoniser costs per batch, on the engine's own masks.

One engine, tiles resident on the device, the flagship shape (batch 16 of 512x512x3).  Per workload:
  * HIP events around rs_op_polygonize on the canvases of one forward (the operator allocates and frees its scratch inside the
    bracket, so this is an upper bound of the kernels' time);
  * wall-clock time of forward + result fetch per batch with the masks as crops, and with polygons instead;
  * the share of instances the kernel left to the host.
Prints one JSON line per workload.

    python tools/polygonize_bench.py [--weights random|trained] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", choices=["random", "trained"], default="random")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--epsilon", type=float, default=0.75)
    args = ap.parse_args()
    import numpy as np
    import torch
    from proj_roadsurf_amd import vectorize as V
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes, synthetic_tiles, train_trained_like
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    if args.weights == "trained":
        W, _ = train_trained_like(spec, 512, steps=args.train_steps)
        tiles = synthetic_scenes(args.batch, 512, 512, 3, seed=555)[0]
    else:
        W = synthetic_weights(spec, seed=0)
        tiles = synthetic_tiles(args.batch, 512, 512, 3, seed=1234)
    tiles = np.ascontiguousarray(tiles[:args.batch])
    n = tiles.shape[0]
    eng = Engine(spec, W, (512, 512, 3), max_batch=n)
    try:
        dets = eng.infer(tiles)
        packed = np.concatenate([d._packed for d in dets if len(d)]) if any(len(d) for d in dets) else np.zeros((0, 512, 64), np.uint8)
        inst = int(packed.shape[0])
        ms_op = []
        flagged = 0
        if inst:
            for _ in range(3 + args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t = V.polygonize_masks_device(packed, 512, 512, args.epsilon)
                b.record()
                torch.cuda.synchronize()
                ms_op.append(a.elapsed_time(b))
            flagged = int(len(t.flagged))
            ms_op = sorted(ms_op[3:])
        ptr = eng.upload_async(tiles)
        eng.sync()
        wall = {}
        for mode in ("crops", "polygons", "crops", "polygons"):
            kw = dict(polygons=True, rdp_epsilon=args.epsilon) if mode == "polygons" else dict(crops=True)
            for _ in range(3):
                eng.infer_device(ptr, n); eng.fetch_async(n, **kw); eng.fetch_wait(n)
            t0 = time.perf_counter()
            for _ in range(args.iters):
                eng.infer_device(ptr, n); eng.fetch_async(n, **kw); eng.fetch_wait(n)
            wall.setdefault(mode, []).append(1e3 * (time.perf_counter() - t0) / args.iters)
        print(json.dumps({"weights": args.weights, "batch": n, "instances_per_batch": inst, "flagged": flagged,
                          "flagged_share": flagged / max(inst, 1), "rdp_epsilon": args.epsilon,
                          "op_ms_incl_upload_and_scratch_median": ms_op[len(ms_op) // 2] if ms_op else None, "op_ms_min": ms_op[0] if ms_op else None,
                          "forward_plus_fetch_wall_ms_per_batch": wall}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
