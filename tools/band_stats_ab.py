#!/usr/bin/env python3
"""What the band histograms behind the forward cost, against the numpy route they replace.

    python tools/band_stats_ab.py [--tile 512] [--batch 16] [--labels 6] [--batches 6] [--host-batches 1] [--windows 3] [--cli-tiles 96] [--out DIR]

One process, one inference engine (synthetic weights).  Arms, each one batch at a time (upload, forward, result fetch as mask crops, wait):
  forward   nothing else: what a batch costs without the histograms;
  device    ``Engine.band_hist(n, labels, wait=False)`` behind the fetch: label rasteriser and ``band_hist_kernel`` on the copy stream,
            one copy of the histograms;
  host      ``band_stats.band_hist_host`` on the batch's tiles on top of the same forward: ``raster_vote.label_rasters`` and ``np.bincount``.
After one warm-up batch per arm, ``windows`` windows of ``batches`` batches are timed per arm in a rotating order.  The labels are
``labels`` strips per tile, 8 to 24 px wide, crossing the tile at random angles (tools/road_votes_ab.py's).  The stage itself -- the
operator ``rs_op_band_hist`` with its clearing memset plus the copy of the histograms into pinned memory -- is also timed alone with HIP
events, in ``windows`` windows of 20 back-to-back calls, on the realistic labels and on the worst case (uniform tiles, one full-tile
label each: every pixel of a wave in one bin); it runs on the copy stream and is no entry of ``Engine.stage_times``.  ``--cli-tiles N``
(0: skip) writes a dataset of N tiles with those labels and times ``make_detections`` with and without ``--road-stats`` on it,
alternating.  Prints one JSON line and writes it to DIR/band_stats_ab.json."""
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


def cli_runs(tiles, labels, T, batch, repeats):
    """``make_detections`` on a dataset of these tiles and labels, with and without --road-stats, alternating: seconds per run."""
    import yaml
    from PIL import Image
    from proj_roadsurf_amd import make_detections
    times = {"plain": [], "road_stats": []}
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
                             "segmentation": [np.clip(r, -8.0, T + 8.0).tolist() for r in rings]})
        cats = [{"id": 1, "name": "artificial"}, {"id": 2, "name": "natural"}]
        json.dump({"images": images, "annotations": anns, "categories": cats}, open(os.path.join(wd, "COCO_val.json"), "w"))
        yaml.safe_dump({"MODEL": {"ROI_HEADS": {"NUM_CLASSES": 2}}}, open(os.path.join(tmp, "d2.yaml"), "w"))
        cfg = {"make_detections.py": {"working_directory": wd, "log_subfolder": "logs", "COCO_files": {"val": "COCO_val.json"},
                                      "detectron2_config_file": os.path.join(tmp, "d2.yaml"), "model_weights": {"pth_file": "none.pth"},
                                      "rdp_simplification": {"enabled": True, "epsilon": 0.75}, "score_lower_threshold": 0.05}}
        yaml.safe_dump(cfg, open(os.path.join(tmp, "config.yaml"), "w"))
        common = [os.path.join(tmp, "config.yaml"), "--synthetic-weights", "--batch", str(batch), "--tagged-samples", "0"]
        cwd = os.getcwd()
        try:
            for r in range(repeats + 1):                         # run 0 of either arm warms the code objects and the page cache
                for arm in (("plain", "road_stats") if r % 2 == 0 else ("road_stats", "plain")):
                    t0 = time.perf_counter()
                    rc = make_detections.main(common + (["--road-stats"] if arm == "road_stats" else []))
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
    ap.add_argument("--cli-tiles", type=int, default=96, help="tiles of the make_detections dataset (0: skip that measurement)")
    ap.add_argument("--cli-repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("band_stats_ab.py measures on a HIP device; none is visible")
    from proj_roadsurf_amd import band_stats as BS
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
    eng = Engine(spec, W, (T, T, C), max_batch=B)
    try:
        def batch(arm, k):
            tl, lb = tiles[k * B:(k + 1) * B], labels[k * B:(k + 1) * B]
            eng.infer_device(eng.upload_async(np.ascontiguousarray(tl)), B)
            eng.fetch_async(B)
            if arm == "device":
                fits = eng.band_hist(B, lb, wait=False)
                eng.fetch_wait(B)
                return eng.band_hist_wait(B) if fits else None
            eng.fetch_wait(B)
            return BS.band_hist_host(tl, lb) if arm == "host" else None

        def window(arm):
            nb = min(n_b, args.host_batches) if arm == "host" else n_b
            t0 = time.perf_counter()
            for k in range(nb):
                batch(arm, k)
            return (time.perf_counter() - t0) / nb
        first = {arm: batch(arm, 0) for arm in ARMS}                  # warm-up: every kernel, shape and lazy buffer of the timed runs
        same = all(np.array_equal(d, h) for d, h in zip(first["device"], first["host"]))
        times = {arm: [] for arm in ARMS}
        for r in range(args.windows):
            for i in range(len(ARMS)):
                arm = ARMS[(r + i) % len(ARMS)]
                times[arm].append(window(arm))
        host_alone = []                                               # the numpy route without the forward around it
        for r in range(args.windows):
            t0 = time.perf_counter()
            BS.band_hist_host(tiles[:B], labels[:B])
            host_alone.append(time.perf_counter() - t0)
        fallbacks = eng.band_fallbacks
    finally:
        eng.close()

    # the stage alone: operator (memset + kernel) and the copy of its table into pinned memory, HIP events around back-to-back calls
    lib = load_library()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def stage(tl, packed, first_of):
        n_inst = int(packed.shape[0])
        t_tiles, t_lab, t_first = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (tl, packed, first_of))
        hist = torch.zeros((n_inst, C, 256), dtype=torch.int32, device=dev)
        pinned = torch.zeros((n_inst, C, 256), dtype=torch.int32).pin_memory()

        def call(copy):
            rc = lib.rs_op_band_hist(t_tiles.data_ptr(), t_lab.data_ptr(), t_first.data_ptr(), B, n_inst, T, C, hist.data_ptr(), stream)
            assert rc == 0, lib.rs_last_error().decode()
            if copy:
                pinned.copy_(hist, non_blocking=True)

        def timed(copy, reps=20):
            call(copy)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call(copy)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps
        out = {"kernel_ms_windows": [round(timed(False), 4) for _ in range(args.windows)],
               "kernel_and_copy_ms_windows": [round(timed(True), 4) for _ in range(args.windows)]}
        want = BS.band_hist_library_host(tl, packed, first_of)
        out["equals_host_restatement"] = bool(np.array_equal(pinned.numpy().view(np.uint32), want))
        out["instances"], out["pixels_counted"] = n_inst, int(want[:, 0].sum())
        return out
    real_packed = np.concatenate([RV.label_rasters(l, T, T) for l in labels[:B]])
    real_first = (np.arange(B + 1) * args.labels).astype(np.int32)
    realistic = stage(tiles[:B], real_packed, real_first)
    uniform = np.empty((B, T, T, C), np.uint8)
    uniform[...] = np.array([90, 120, 60], np.uint8)[:C]
    full = np.full((B, T, (T + 7) // 8), 0xFF, np.uint8)
    if T % 8:
        full[:, :, -1] = (1 << (T % 8)) - 1
    worst = stage(uniform, full, np.arange(B + 1, dtype=np.int32))

    out = {"tool": "tools/band_stats_ab.py", "device": torch.cuda.get_device_name(0), "tile": T, "batch": B, "channels": C,
           "labels_per_tile": args.labels, "batches_per_window": n_b, "host_batches_per_window": min(n_b, args.host_batches),
           "windows": args.windows, "precision": spec.precision, "tables_identical": bool(same), "fallback_batches": int(fallbacks),
           "host_route_alone_ms_windows": [round(1e3 * x, 2) for x in host_alone], "stage_realistic": realistic, "stage_worst_case": worst}
    for arm in ARMS:
        out[f"{arm}_ms_per_batch_windows"] = [round(1e3 * x, 3) for x in times[arm]]
        out[f"{arm}_ms_per_batch_median"] = 1e3 * statistics.median(times[arm])
    fwd = out["forward_ms_per_batch_median"]
    out["stage_realistic_over_forward"] = statistics.median(realistic["kernel_and_copy_ms_windows"]) / fwd
    out["stage_worst_case_over_forward"] = statistics.median(worst["kernel_and_copy_ms_windows"]) / fwd
    if args.cli_tiles > 0:
        cli = cli_runs(tiles[:args.cli_tiles], labels[:args.cli_tiles], T, B, args.cli_repeats)
        out["cli_tiles"] = args.cli_tiles
        out["cli_plain_s_runs"] = [round(x, 3) for x in cli["plain"]]
        out["cli_road_stats_s_runs"] = [round(x, 3) for x in cli["road_stats"]]
    print("  ".join(f"{arm} {out[f'{arm}_ms_per_batch_median']:.2f} ms" for arm in ARMS) + f" per batch of {B} tiles; stage alone "
          f"{realistic['kernel_and_copy_ms_windows']} ms (realistic), {worst['kernel_and_copy_ms_windows']} ms (worst case); tables identical: {same}",
          file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "band_stats_ab.json"), "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
