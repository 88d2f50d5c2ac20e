#!/usr/bin/env python3
"""A/B of the three validation-AP paths of train_model: ``--val-ap host`` against ``device`` against ``device-match``.

    python tools/val_ap_ab.py [--tiles 32] [--tile 512] [--batch 8] [--rounds 5] [--weights random|trained] [--out DIR]

One process, one inference engine.  An evaluation here is what ``train_model.validation_ap`` does per rank with N validation tiles
already decoded: per chunk of ``batch`` tiles ``train_model.validation_chunk`` (the forward, then either the masks copied back,
unpacked and the ground truth rasterised on the host, or ``Engine.eval_counts``), then ``coco_eval.match_images`` for bbox and segm
over all images; in the third mode ``train_model.validation_chunk_records`` (``Engine.eval_matches``: the matching runs on the GPU too and
the host only unpacks flag bits).  Two figures per evaluation: the wall time, and the host time spent matching (``match_images``, or
the unpacking of the tables).  The host and device modes are the code paths of the parent commit and so the baseline.  After one
warm-up evaluation per mode, ``rounds`` evaluations are timed in a rotating order, and the match records of the modes are compared.
The tiles and their ground truth are synthetic.synthetic_scenes'.  ``--weights random``: synthetic weights, the saturated detector
(every slot of every tile holds a detection); ``trained``: ``synthetic.train_trained_like``, a handful of detections per tile.  Prints
one JSON line and writes it to DIR/val_ap_ab_<weights>.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("host", "device", "device-match")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tiles", type=int, default=32, help="validation tiles per evaluation")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8, help="tiles per chunk (train_model: IMS_PER_BATCH / ranks)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--weights", choices=("random", "trained"), default="random")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("val_ap_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.coco_eval import match_images
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes, train_trained_like
    from proj_roadsurf_amd.train_model import validation_chunk, validation_chunk_records
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    T, N, B = args.tile, args.tiles, args.batch
    W = train_trained_like(spec, T, steps=args.train_steps)[0] if args.weights == "trained" else synthetic_weights(spec, seed=0)
    tiles, boxes, classes, polys = synthetic_scenes(N, T, T, 3, seed=4321)
    recs = [{"boxes": np.asarray(boxes[i], np.float64), "classes": np.asarray(classes[i], np.int64), "polygons": polys[i]} for i in range(N)]
    eng = Engine(spec, W, (T, T, 3), max_batch=B)
    try:
        def evaluation(mode):
            t0 = time.perf_counter()
            fell = 0
            if mode == "device-match":
                out = {"bbox": [], "segm": []}
                eng.eval_unpack_s = 0.0
                for k in range(0, N, B):
                    rb, rs, fb = validation_chunk_records(eng, spec, recs[k:k + B], tiles[k:k + B])
                    out["bbox"] += rb; out["segm"] += rs; fell += int(fb)
                t2 = time.perf_counter()
                match_s, dets = eng.eval_unpack_s, sum(len(r[key][0]) for r in out["bbox"] for key in r if key[1] == "all")
            else:
                gts, dts = [], []
                for k in range(0, N, B):
                    g, d, fb = validation_chunk(eng, spec, recs[k:k + B], tiles[k:k + B], mode)
                    gts += g; dts += d; fell += int(fb)
                t1 = time.perf_counter()
                out = {kind: match_images(gts, dts, spec.num_classes, kind, spec.detections_per_image) for kind in ("bbox", "segm")}
                t2 = time.perf_counter()
                match_s, dets = t2 - t1, sum(len(d["scores"]) for d in dts)
            return {"total_s": t2 - t0, "match_s": match_s, "fallbacks": fell, "detections": dets}, out
        first = {m: evaluation(m) for m in MODES}       # warm-up: every kernel, shape and lazy buffer of the timed runs

        def same(a, b):
            return all(ra.keys() == rb.keys() and all(np.array_equal(np.asarray(x), np.asarray(y)) for key in ra for x, y in zip(ra[key], rb[key]))
                       for kind in ("bbox", "segm") for ra, rb in zip(first[a][1][kind], first[b][1][kind]))
        times = {m: [] for m in MODES}
        for r in range(args.rounds):
            for i in range(len(MODES)):
                m = MODES[(r + i) % len(MODES)]
                times[m].append(evaluation(m)[0])
        out = {"tool": "tools/val_ap_ab.py", "device": torch.cuda.get_device_name(0), "weights": args.weights, "tile": T, "tiles": N, "chunk": B,
               "rounds": args.rounds, "precision": spec.precision, "detections_per_evaluation": first["host"][0]["detections"],
               "detections_per_tile_mean": first["host"][0]["detections"] / N,
               "ground_truths_per_tile_mean": sum(len(r["classes"]) for r in recs) / N,
               "ground_truth_vertices_mean": float(np.mean([p.size / 2 for r in recs for inst in r["polygons"] for p in inst])),
               "match_records_identical": bool(same("host", "device") and same("host", "device-match")),
               "fallback_chunks": {m: first[m][0]["fallbacks"] for m in MODES}}
        for m in MODES:
            for key in ("total_s", "match_s"):
                v = [t[key] for t in times[m]]
                out[f"{m}_{key}_runs"] = [round(x, 5) for x in v]
                out[f"{m}_{key}_median"] = statistics.median(v)
                out[f"{m}_{key}_min"], out[f"{m}_{key}_max"] = min(v), max(v)
        print("  ".join(f"{m} {out[f'{m}_total_s_median']:.3f} s (matching {out[f'{m}_match_s_median'] * 1e3:.1f} ms)" for m in MODES)
              + f" per evaluation of {N} tiles ({out['detections_per_tile_mean']:.1f} detections, {out['ground_truths_per_tile_mean']:.1f} ground truths "
              f"per tile); records identical: {out['match_records_identical']}", file=sys.stderr, flush=True)
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"val_ap_ab_{args.weights}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
