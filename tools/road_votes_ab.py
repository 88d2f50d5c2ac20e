#!/usr/bin/env python3
"""A/B of the two routes from a batch of tiles to its road vote tables.

    python tools/road_votes_ab.py [--tile 512] [--batch 16] [--labels 8] [--batches 6] [--host-batches 1] [--windows 3] [--weights random|trained] [--out DIR]

One process, one inference engine.  Three arms, each one batch at a time (upload, forward, result fetch as mask crops, wait):
  forward   nothing else: what a batch costs without any vote;
  device    ``Engine.road_votes(n, labels, wait=False)`` behind the fetch: label rasteriser, pair counts and vote on the copy stream,
            only the vote tables travel;
  host      the route of the parent commit to the same numbers: the fetched masks, ``raster_vote.label_rasters``, the numpy popcounts
            (``oracle.host_tail_oracle.overlap_counts``) and the Python vote ``raster_vote.weighted_scores``.
After one warm-up batch per arm, ``windows`` windows of ``batches`` batches are timed per arm in a rotating order.  The labels are
``labels`` strips per tile, 8 to 24 px wide, crossing the tile at random angles.  The two kernels behind the device arm are also timed
alone, with HIP events, on tables of the engine's shapes (``rs_op_mask_pair_counts`` on the batch's own masks and label rasters,
``rs_op_road_votes`` on its counts): they run on the copy stream and are no entries of ``Engine.stage_times``.  ``--weights random``:
synthetic weights, the saturated detector (every slot of every tile holds a detection); ``trained``: ``synthetic.train_trained_like``,
a handful of detections per tile.  Prints one JSON line and writes it to DIR/road_votes_ab_<weights>.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("forward", "device", "host")


def strips(rng, n_tiles, per_tile, T):
    """per_tile road-like labels per tile: rectangles of width 8..24 px through a random point at a random angle, long enough to cross
    the tile (the rasteriser clips them)."""
    out = []
    for _ in range(n_tiles):
        labs = []
        for _ in range(per_tile):
            cx, cy, a, w = rng.uniform(0, T), rng.uniform(0, T), rng.uniform(0, np.pi), rng.uniform(8, 24)
            d, nrm = np.array([np.cos(a), np.sin(a)]) * 2 * T, np.array([-np.sin(a), np.cos(a)]) * w / 2
            c = np.array([cx, cy])
            labs.append([np.concatenate([c - d - nrm, c + d - nrm, c + d + nrm, c - d + nrm])])
        out.append(labs)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--labels", type=int, default=8, help="road labels per tile")
    ap.add_argument("--batches", type=int, default=6, help="batches per window")
    ap.add_argument("--host-batches", type=int, default=1, help="batches per window of the host arm (its numpy popcounts take seconds per batch)")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.3)
    ap.add_argument("--weights", choices=("random", "trained"), default="random")
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("road_votes_ab.py measures on a HIP device; none is visible")
    from oracle.host_tail_oracle import overlap_counts
    from proj_roadsurf_amd import raster_vote as RV
    from proj_roadsurf_amd.engine import Engine, load_library
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes, train_trained_like
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    T, B, K = args.tile, args.batch, 2
    W = train_trained_like(spec, T, steps=args.train_steps)[0] if args.weights == "trained" else synthetic_weights(spec, seed=0)
    n_b = args.batches
    tiles = synthetic_scenes(B * n_b, T, T, 3, seed=4321)[0]
    labels = strips(np.random.default_rng(7), B * n_b, args.labels, T)
    ids = [[f"r{t}_{g}" for g in range(args.labels)] for t in range(B * n_b)]
    eng = Engine(spec, W, (T, T, 3), max_batch=B)
    try:
        def batch(arm, k):
            tl, lb = tiles[k * B:(k + 1) * B], labels[k * B:(k + 1) * B]
            eng.infer_device(eng.upload_async(np.ascontiguousarray(tl)), B)
            eng.fetch_async(B)
            if arm == "device":
                fits = eng.road_votes(B, lb, args.threshold, wait=False)
                res = eng.fetch_wait(B)
                return res, (eng.road_votes_wait(B, False) if fits else None)
            res = eng.fetch_wait(B)
            if arm == "forward":
                return res, None
            rows = []
            for i, r in enumerate(res):
                lp = RV.label_rasters(lb[i], T, T)
                inter, area = overlap_counts(r._packed, lp)
                rows.append(RV.weighted_scores(inter, area, r.scores, r.pred_classes, ids[k * B + i]))
            return res, rows

        def window(arm):
            nb = min(n_b, args.host_batches) if arm == "host" else n_b
            t0 = time.perf_counter()
            for k in range(nb):
                batch(arm, k)
            return (time.perf_counter() - t0) / nb
        first = {arm: batch(arm, 0) for arm in ARMS}                  # warm-up: every kernel, shape and lazy buffer of the timed runs
        # the two routes give the same numbers: the device tables against the sums of the host rows
        same = True
        for i in range(B):
            ws, wa, pairs, area = first["device"][1][i]
            hw, ha, hp = np.zeros_like(ws), np.zeros_like(wa), np.zeros_like(pairs)
            for r in first["host"][1][i]:
                if r["score"] >= args.threshold:
                    g = int(str(r["OBJECTID"]).split("_")[1])
                    hw[g, r["det_class"]] += r["weighted_score"]; ha[g, r["det_class"]] += r["area_pred_in_label"]; hp[g, r["det_class"]] += 1
            same = same and np.array_equal(ws, hw) and np.array_equal(wa, ha) and np.array_equal(pairs, hp)
        fallbacks = eng.vote_fallbacks
        times = {arm: [] for arm in ARMS}
        for r in range(args.windows):
            for i in range(len(ARMS)):
                arm = ARMS[(r + i) % len(ARMS)]
                times[arm].append(window(arm))
        # the two kernels alone, on this batch's own masks
        lib = load_library()
        res = eng.infer(tiles[:B])
        D = spec.detections_per_image
        det = np.zeros((B, D, T, (T + 7) // 8), np.uint8)
        cnt = np.array([len(r) for r in res], np.int32)
        for i, r in enumerate(res):
            det[i, :len(r)] = r._packed
        lab = np.concatenate([RV.label_rasters(l, T, T) for l in labels[:B]])
        first_of = np.arange(B + 1, dtype=np.int32) * args.labels
        dev = torch.device("cuda")
        t_det, t_lab, t_cnt, t_first = (torch.from_numpy(a).to(dev) for a in (det, lab, cnt, first_of))
        inter = torch.zeros((B, D, 128), dtype=torch.int32, device=dev)
        d_area = torch.zeros((B, D), dtype=torch.int32, device=dev)
        g_area = torch.zeros((B, 128), dtype=torch.int32, device=dev)
        sc = torch.zeros((B, D), dtype=torch.float32, device=dev)
        cl = torch.zeros((B, D), dtype=torch.int32, device=dev)
        for i, r in enumerate(res):
            sc[i, :len(r)] = torch.from_numpy(r.scores).to(dev)
            cl[i, :len(r)] = torch.from_numpy(r.pred_classes.astype(np.int32)).to(dev)
        ws_d = torch.zeros((B, 128, K), dtype=torch.float64, device=dev)
        wa_d = torch.zeros_like(ws_d)
        pr_d = torch.zeros((B, 128, K), dtype=torch.int32, device=dev)

        def timed(fn, reps=20):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps
        stream = torch.cuda.current_stream().cuda_stream
        pair_ms = timed(lambda: lib.rs_op_mask_pair_counts(t_det.data_ptr(), t_cnt.data_ptr(), B, D, t_lab.data_ptr(), t_first.data_ptr(), 128, T,
                                                           inter.data_ptr(), d_area.data_ptr(), g_area.data_ptr(), stream))
        vote_ms = timed(lambda: lib.rs_op_road_votes(sc.data_ptr(), cl.data_ptr(), t_cnt.data_ptr(), t_first.data_ptr(), inter.data_ptr(), g_area.data_ptr(),
                                                     B, K, D, 128, float(args.threshold), ws_d.data_ptr(), wa_d.data_ptr(), pr_d.data_ptr(), stream))
        out = {"tool": "tools/road_votes_ab.py", "device": torch.cuda.get_device_name(0), "weights": args.weights, "tile": T, "batch": B,
               "labels_per_tile": args.labels, "batches_per_window": n_b, "host_batches_per_window": min(n_b, args.host_batches), "windows": args.windows, "precision": spec.precision, "threshold": args.threshold,
               "detections_per_tile_mean": float(np.mean([len(r) for r in first["forward"][0]])),
               "pairs_per_tile_mean": float(np.mean([int(t[2].sum()) for t in first["device"][1]])),
               "tables_identical": bool(same), "fallback_batches": int(fallbacks), "batches_voted": 1 + args.windows * n_b,
               "pair_counts_kernel_ms": pair_ms, "road_vote_kernel_ms": vote_ms}
        for arm in ARMS:
            out[f"{arm}_ms_per_batch_windows"] = [round(1e3 * x, 3) for x in times[arm]]
            out[f"{arm}_ms_per_batch_median"] = 1e3 * statistics.median(times[arm])
        print("  ".join(f"{arm} {out[f'{arm}_ms_per_batch_median']:.2f} ms" for arm in ARMS) + f" per batch of {B} tiles; pair counts {pair_ms:.3f} ms, "
              f"vote {vote_ms:.4f} ms; tables identical: {same}", file=sys.stderr, flush=True)
    finally:
        eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"road_votes_ab_{args.weights}.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
