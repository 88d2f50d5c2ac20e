#!/usr/bin/env python3
"""What the road vote on polygon areas costs behind the forward, against the pixel route and the host restatement, and how far the two
geometries' results are apart.

    python tools/poly_votes_ab.py [--tile 512] [--batch 16] [--labels 6] [--batches 6] [--windows 3] [--thresholds 20] [--cli-tiles 96] [--out DIR]

One process, one inference engine (synthetic weights).  Arms, each one batch at a time (upload, forward, polygons fetch, wait):
  forward    nothing else: what a batch costs with the device polygoniser and no vote;
  polygons   ``Engine.road_votes_sweep(n, labels, thresholds, geometry="polygons", wait=False)`` behind the fetch: label upload,
             ``poly_overlap_kernel``, ``road_vote_area_sweep_kernel`` and five small copies on the copy stream;
  pixels     ``Engine.road_votes_sweep(n, labels, thresholds, wait=False)`` behind the same fetch: label rasteriser, pair counts, sweep;
  host       ``Engine.polygon_vote_host_rows`` on the fetched polygons on top of the same forward (the host restatement, per tile).
After one warm-up batch per arm, ``windows`` windows of ``batches`` batches are timed per arm in a rotating order.  The labels are
``labels`` strips per tile, 8 to 24 px wide, crossing the tile at random angles and CLIPPED to the tile, as the reference's labels are.
The stage itself -- ``rs_op_polygon_overlaps``, ``rs_op_road_votes_area_sweep`` with their clearing memsets, plus the copies of the
three vote tables, the label areas and the flags into pinned memory -- is also timed alone with HIP events on the polygon tables of
the first batch, in ``windows`` windows of 20 back-to-back calls.  Parity: the share of (label, class) cells with a pair in either
geometry whose (pairs, wfrac) differ, and of roads whose final cover differs, at threshold 0.  ``--cli-tiles N`` (0: skip) times
``make_detections --vectorize device --road-votes --road-metrics`` with and without ``--vote-geometry polygons``, alternating.
Prints one JSON line and writes it to DIR/poly_votes_ab.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("forward", "polygons", "pixels", "host")


def clip_to_tile(poly, T):
    """Sutherland-Hodgman of a convex ring (k, 2) against [0, T]^2."""
    pts = [tuple(p) for p in poly]
    for axis, bound, keep_le in ((0, 0.0, False), (0, float(T), True), (1, 0.0, False), (1, float(T), True)):
        out = []
        for i, p in enumerate(pts):
            q = pts[(i + 1) % len(pts)]
            pin = p[axis] <= bound if keep_le else p[axis] >= bound
            qin = q[axis] <= bound if keep_le else q[axis] >= bound
            if pin:
                out.append(p)
            if pin != qin:
                t = (bound - p[axis]) / (q[axis] - p[axis])
                x = [p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])]
                x[axis] = bound
                out.append(tuple(x))
        pts = out
        if not pts:
            return None
    return np.array(pts, np.float64)


def strips(rng, n_tiles, per_tile, T):
    """per_tile road-like labels per tile: strips of width 8..24 px through a random point at a random angle, clipped to the tile."""
    out = []
    for _ in range(n_tiles):
        labs = []
        while len(labs) < per_tile:
            cx, cy, a, w = rng.uniform(0, T), rng.uniform(0, T), rng.uniform(0, np.pi), rng.uniform(8, 24)
            d, nrm = np.array([np.cos(a), np.sin(a)]) * 2 * T, np.array([-np.sin(a), np.cos(a)]) * w / 2
            c = np.array([cx, cy])
            ring = clip_to_tile(np.stack([c - d - nrm, c + d - nrm, c + d + nrm, c - d + nrm]), T)
            if ring is not None and len(ring) >= 3:
                labs.append([ring.reshape(-1)])
        out.append(labs)
    return out


def cli_runs(tiles, labels, T, batch, repeats):
    import yaml
    from PIL import Image
    from proj_roadsurf_amd import make_detections
    times = {"pixels": [], "polygons": []}
    with tempfile.TemporaryDirectory() as tmp:
        wd = os.path.join(tmp, "outputs")
        os.makedirs(os.path.join(wd, "val-images"))
        images, anns = [], []
        for i, t in enumerate(tiles):
            fn = f"val-images/18_{100 + i}_200.tif"
            Image.fromarray(np.ascontiguousarray(t[:, :, ::-1])).save(os.path.join(wd, fn))
            images.append({"id": i, "file_name": fn, "width": T, "height": T})
            for g, rings in enumerate(labels[i]):
                anns.append({"id": len(anns), "image_id": i, "category_id": 1 + g % 2, "iscrowd": 0, "road_id": f"r{(i // 2) * 100 + g}",
                             "segmentation": [r.tolist() for r in rings]})
        cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
        json.dump({"images": images, "annotations": anns, "categories": cats}, open(os.path.join(wd, "COCO_val.json"), "w"))
        yaml.safe_dump({"MODEL": {"ROI_HEADS": {"NUM_CLASSES": 2}}}, open(os.path.join(tmp, "d2.yaml"), "w"))
        cfg = {"make_detections.py": {"working_directory": wd, "log_subfolder": "logs", "COCO_files": {"val": "COCO_val.json"},
                                      "detectron2_config_file": os.path.join(tmp, "d2.yaml"), "model_weights": {"pth_file": "none.pth"},
                                      "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05}}
        yaml.safe_dump(cfg, open(os.path.join(tmp, "config.yaml"), "w"))
        common = [os.path.join(tmp, "config.yaml"), "--synthetic-weights", "--batch", str(batch), "--tagged-samples", "0", "--vectorize", "device",
                  "--road-votes", "--road-metrics"]
        cwd = os.getcwd()
        try:
            for r in range(repeats + 1):                         # run 0 of either arm warms the code objects and the page cache
                for arm in (("pixels", "polygons") if r % 2 == 0 else ("polygons", "pixels")):
                    t0 = time.perf_counter()
                    rc = make_detections.main(common + (["--vote-geometry", "polygons"] if arm == "polygons" else []))
                    os.chdir(cwd)
                    if rc != 0:
                        raise SystemExit(f"make_detections returned {rc}")
                    if r:
                        times[arm].append(time.perf_counter() - t0)
        finally:
            os.chdir(cwd)
    return times


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--labels", type=int, default=6, help="road labels per tile")
    ap.add_argument("--batches", type=int, default=6, help="batches per window")
    ap.add_argument("--host-batches", type=int, default=1, help="batches per window of the host arm")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--thresholds", type=int, default=20)
    ap.add_argument("--cli-tiles", type=int, default=96, help="tiles of the make_detections dataset (0: skip that measurement)")
    ap.add_argument("--cli-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("poly_votes_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd import raster_vote as RV
    from proj_roadsurf_amd.engine import Engine, load_library
    from proj_roadsurf_amd.spec import EngineSpec
    from proj_roadsurf_amd.synthetic import synthetic_scenes
    from proj_roadsurf_amd.weights import synthetic_weights

    spec = EngineSpec(num_classes=2)
    T, B, C = args.tile, args.batch, 3
    W = synthetic_weights(spec, seed=0)
    n_b = args.batches
    n_tiles = max(B * n_b, args.cli_tiles)
    tiles = synthetic_scenes(n_tiles, T, T, C, seed=4321)[0]
    labels = strips(np.random.default_rng(7), n_tiles, args.labels, T)
    thr = np.linspace(0.0, 0.95, args.thresholds)
    eng = Engine(spec, W, (T, T, C), max_batch=B)
    try:
        def batch(arm, k):
            tl, lb = tiles[k * B:(k + 1) * B], labels[k * B:(k + 1) * B]
            eng.infer_device(eng.upload_async(np.ascontiguousarray(tl)), B)
            eng.fetch_async(B, polygons=True, rdp_epsilon=0.75)
            if arm == "polygons":
                eng.road_votes_sweep(B, lb, thr, wait=False, geometry="polygons")
                return eng.road_votes_polygons_wait(B)
            if arm == "pixels":
                fits = eng.road_votes_sweep(B, lb, thr, wait=False)
                res = eng.fetch_wait(B)
                return [(r,) + row for r, row in zip(res, eng.road_votes_sweep_wait(B, False))] if fits else None
            res = eng.fetch_wait(B)
            return [(r,) + row for r, row in zip(res, eng.polygon_vote_host_rows(res, lb, thr))] if arm == "host" else res

        def window(arm):
            nb = min(n_b, args.host_batches) if arm == "host" else n_b
            t0 = time.perf_counter()
            for k in range(nb):
                batch(arm, k)
            return (time.perf_counter() - t0) / nb
        first = {arm: batch(arm, 0) for arm in ARMS}                  # warm-up: every kernel, shape and lazy buffer of the timed runs
        same = all(all(np.array_equal(a, b) for a, b in zip(d[1:], h[1:])) for d, h in zip(first["polygons"], first["host"]))
        times = {arm: [] for arm in ARMS}
        for r in range(args.windows):
            for i in range(len(ARMS)):
                arm = ARMS[(r + i) % len(ARMS)]
                times[arm].append(window(arm))
        # parity over every batch: cells and roads
        cells = differ = 0
        rows_pix, rows_pol, ids = [], [], []
        for k in range(n_b):
            pol, pix = batch("polygons", k), batch("pixels", k)
            for i, (a, b) in enumerate(zip(pol, pix)):
                live = (a[3][0] > 0) | (b[3][0] > 0)
                cells += int(live.sum())
                differ += int((live & ((a[3][0] != b[3][0]) | (a[2][0] != b[2][0]))).sum())
                rows_pol.append(RV.sweep_slice(a[1:], 0))
                rows_pix.append(RV.sweep_slice(b[1:], 0))
                ids.append([f"r{((k * B + i) // 2) * 100 + g}" for g in range(len(labels[k * B + i]))])
        cover_pol = {r["road_id"]: r["cover_type"] for r in RV.reduce_votes(rows_pol, ids)}
        cover_pix = {r["road_id"]: r["cover_type"] for r in RV.reduce_votes(rows_pix, ids)}
        fallbacks = eng.vote_fallbacks
        stage_res = first["forward"]
    finally:
        eng.close()

    # the stage alone on the first batch's polygon tables: two operators and five copies, HIP events around back-to-back calls
    lib = load_library()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    det = RV.stack_polygon_tables([r._polygons for r in stage_res])
    pool = RV.pack_label_pool(labels[:B])
    D = det["header"].shape[1]
    scores, classes = np.zeros((B, D), np.float32), np.zeros((B, D), np.int32)
    for i, r in enumerate(stage_res):
        scores[i, :len(r)], classes[i, :len(r)] = r.scores, r.pred_classes
    dts = (np.int32, np.int32, np.int32, np.int16, np.int32, np.int32, np.int32, np.int32, np.int32, np.float64)
    t_in = [torch.from_numpy(np.ascontiguousarray({**det, **pool}[k], dt)).to(dev) for k, dt in zip(RV.POLY_TABLE_KEYS, dts)]
    t_sc, t_cl = torch.from_numpy(scores).to(dev), torch.from_numpy(classes).to(dev)
    Tn = int(thr.size)
    frac = torch.zeros((B, D, 128), dtype=torch.float64, device=dev)
    area = torch.zeros((B, 128), dtype=torch.float64, device=dev)
    flg = torch.zeros((B,), dtype=torch.int32, device=dev)
    outs = [torch.zeros((B, Tn, 128, 2), dtype=dt, device=dev) for dt in (torch.float64, torch.float64, torch.int32)]
    pinned = [torch.zeros_like(o, device="cpu").pin_memory() for o in outs + [area, flg]]
    import ctypes as Ct
    vp = Ct.c_void_p
    lib.rs_op_polygon_overlaps.argtypes = [vp] * 10 + [Ct.c_int] * 4 + [vp] * 4
    lib.rs_op_road_votes_area_sweep.argtypes = [vp] * 5 + [Ct.c_int] * 4 + [vp, Ct.c_int] + [vp] * 4

    def call(copy, sweep=True):
        rc = lib.rs_op_polygon_overlaps(*[a.data_ptr() for a in t_in], B, D, 128, 0, frac.data_ptr(), area.data_ptr(), flg.data_ptr(), stream)
        assert rc == 0, lib.rs_last_error().decode()
        if sweep:
            rc = lib.rs_op_road_votes_area_sweep(t_sc.data_ptr(), t_cl.data_ptr(), t_in[4].data_ptr(), t_in[5].data_ptr(), frac.data_ptr(), B, 2, D, 128,
                                                 thr.ctypes.data, Tn, *[o.data_ptr() for o in outs], stream)
            assert rc == 0, lib.rs_last_error().decode()
        if copy:
            for p, o in zip(pinned, outs + [area, flg]):
                p.copy_(o, non_blocking=True)

    def timed(copy, sweep=True, reps=20):
        call(copy, sweep)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(copy, sweep)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps
    stage = {"overlap_kernel_ms_windows": [round(timed(False, False), 4) for _ in range(args.windows)],
             "overlap_and_sweep_ms_windows": [round(timed(False), 4) for _ in range(args.windows)],
             "stage_with_copies_ms_windows": [round(timed(True), 4) for _ in range(args.windows)],
             "detections": int(det["det_count"].sum()), "detection_vertices": int(det["xy"].shape[0]), "labels": int(pool["tile_first"][-1])}
    host_alone = []
    for r in range(args.windows):
        t0 = time.perf_counter()
        RV.polygon_overlaps_host({**det, **pool}, gt_cap=128)
        host_alone.append(time.perf_counter() - t0)

    out = {"tool": "tools/poly_votes_ab.py", "device": torch.cuda.get_device_name(0), "tile": T, "batch": B, "labels_per_tile": args.labels,
           "thresholds": Tn, "batches_per_window": n_b, "host_batches_per_window": min(n_b, args.host_batches), "windows": args.windows,
           "precision": spec.precision, "tables_identical_to_host_route": bool(same), "fallback_batches": int(fallbacks), "stage": stage,
           "host_restatement_overlaps_ms_windows": [round(1e3 * x, 2) for x in host_alone],
           "parity": {"cells_with_a_pair": cells, "cells_that_differ": differ, "roads": len(cover_pix),
                      "roads_whose_cover_differs": sum(cover_pix[r] != cover_pol[r] for r in cover_pix)}}
    for arm in ARMS:
        out[f"{arm}_ms_per_batch_windows"] = [round(1e3 * x, 3) for x in times[arm]]
        out[f"{arm}_ms_per_batch_median"] = 1e3 * statistics.median(times[arm])
    out["stage_over_forward"] = statistics.median(stage["stage_with_copies_ms_windows"]) / out["forward_ms_per_batch_median"]
    if args.cli_tiles > 0:
        cli = cli_runs(tiles[:args.cli_tiles], labels[:args.cli_tiles], T, B, args.cli_repeats)
        out["cli_tiles"] = args.cli_tiles
        out["cli_pixels_s_runs"] = [round(x, 3) for x in cli["pixels"]]
        out["cli_polygons_s_runs"] = [round(x, 3) for x in cli["polygons"]]
    print("  ".join(f"{arm} {out[f'{arm}_ms_per_batch_median']:.2f} ms" for arm in ARMS) + f" per batch of {B} tiles; stage alone "
          f"{stage['stage_with_copies_ms_windows']} ms; tables identical to the host route: {same}; parity {out['parity']}", file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "poly_votes_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
