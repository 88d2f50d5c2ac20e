#!/usr/bin/env python3
"""A/B of the two validation-AP paths of train_model: ``--val-ap host`` against ``--val-ap device``.

    python tools/val_ap_ab.py [--tiles 32] [--tile 512] [--batch 8] [--rounds 5] [--out DIR]

One process, one inference engine.  An evaluation here is what ``train_model.validation_ap`` does per rank with N validation tiles
already decoded: per chunk of ``batch`` tiles ``train_model.validation_chunk`` (the forward, then either the masks copied back,
unpacked and the ground truth rasterised on the host, or ``Engine.eval_counts``), then ``coco_eval.match_images`` for bbox and segm
over all images.  The host mode is the code path of the parent commit and so the baseline.  After one warm-up evaluation per mode,
``rounds`` evaluations are timed alternately -- host, device, device, host, ... -- and the match records of the two modes are compared.
The tiles and their ground truth are synthetic.synthetic_scenes'; the weights are synthetic, so the detections are what random
weights give (their number per tile is reported: the host's IoU cost grows with it).  Prints one JSON line and writes it to
DIR/val_ap_ab.json."""
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
    ap.add_argument("--tiles", type=int, default=32, help="validation tiles per evaluation")
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8, help="tiles per chunk (train_model: IMS_PER_BATCH / ranks)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("val_ap_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd.coco_eval import match_images
    from proj_roadsurf_amd.engine import Engine
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.train_model import validation_chunk
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    T, N, B = args.tile, args.tiles, args.batch
    tiles, boxes, classes, polys = synthetic_scenes(N, T, T, 3, seed=4321)
    recs = [{"boxes": np.asarray(boxes[i], np.float64), "classes": np.asarray(classes[i], np.int64), "polygons": polys[i]} for i in range(N)]
    eng = Engine(spec, W, (T, T, 3), max_batch=B)
    try:
        def evaluation(mode):
            t0 = time.perf_counter()
            gts, dts, fell = [], [], 0
            for k in range(0, N, B):
                g, d, fb = validation_chunk(eng, spec, recs[k:k + B], tiles[k:k + B], mode)
                gts += g; dts += d; fell += int(fb)
            t1 = time.perf_counter()
            out = {kind: match_images(gts, dts, spec.num_classes, kind, spec.detections_per_image) for kind in ("bbox", "segm")}
            t2 = time.perf_counter()
            return {"total_s": t2 - t0, "chunks_s": t1 - t0, "match_s": t2 - t1, "fallbacks": fell, "detections": sum(len(d["scores"]) for d in dts)}, out
        first = {m: evaluation(m) for m in ("host", "device")}       # warm-up: every kernel, shape and lazy buffer of the timed runs
        same = all(np.array_equal(np.asarray(x), np.asarray(y))
                   for kind in ("bbox", "segm") for ra, rb in zip(first["host"][1][kind], first["device"][1][kind])
                   for key in ra for x, y in zip(ra[key], rb[key])) and all(
                       ra.keys() == rb.keys() for kind in ("bbox", "segm") for ra, rb in zip(first["host"][1][kind], first["device"][1][kind]))
        times = {m: [] for m in first}
        for r in range(args.rounds):
            for m in (("host", "device") if r % 2 == 0 else ("device", "host")):
                times[m].append(evaluation(m)[0])
        out = {"tool": "tools/val_ap_ab.py", "device": torch.cuda.get_device_name(0), "tile": T, "tiles": N, "chunk": B, "rounds": args.rounds,
               "precision": spec.precision, "detections_per_evaluation": first["host"][0]["detections"],
               "detections_per_tile_mean": first["host"][0]["detections"] / N,
               "ground_truths_per_tile_mean": sum(len(r["classes"]) for r in recs) / N,
               "ground_truth_vertices_mean": float(np.mean([p.size / 2 for r in recs for inst in r["polygons"] for p in inst])),
               "match_records_identical": bool(same), "device_fallback_chunks": first["device"][0]["fallbacks"]}
        for m in times:
            for key in ("total_s", "chunks_s", "match_s"):
                v = [t[key] for t in times[m]]
                out[f"{m}_{key}_runs"] = [round(x, 5) for x in v]
                out[f"{m}_{key}_median"] = statistics.median(v)
                out[f"{m}_{key}_min"] = min(v)
        out["host_over_device_total_median"] = out["host_total_s_median"] / out["device_total_s_median"]
        print(f"host {out['host_total_s_median']:.3f} s  device {out['device_total_s_median']:.3f} s per evaluation of {N} tiles "
              f"({out['detections_per_tile_mean']:.1f} detections, {out['ground_truths_per_tile_mean']:.1f} ground truths per tile); "
              f"records identical: {same}", file=sys.stderr, flush=True)
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "val_ap_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
