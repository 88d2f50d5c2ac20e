#!/usr/bin/env python3
"""Process-level drop-in for the STDL object-detector's ``make_detections.py`` as proj-roadsurf invokes it
(R:README.md:78): same argv (one YAML path), same YAML section ``make_detections.py:``
(R:config/config_obj_detec.yaml:74-90), same output files
(``<dataset>_detections_at_<thr>_threshold.gpkg`` with columns ``score``, ``det_class``, ``geometry`` --
R:config/config_obj_detec.yaml:100-103; plus a ``.geojson`` twin).

    python -m proj_roadsurf_amd.make_detections config/config_obj_detec.yaml
    python -m torch.distributed.run --nproc-per-node 8 -m proj_roadsurf_amd.make_detections config/config_obj_detec.yaml

Host Python only does what BASELINE.json:north_star leaves on the host: YAML/COCO-JSON I/O, tile decode,
weight loading, mask polygonisation and file writing.  The detector itself is ``librs_engine.so``.
With several ranks (RANK/WORLD_SIZE in the environment) the tile list of every dataset is sharded, one
GPU per rank, no collectives on the data path; rank 0 gathers the features and writes the files.
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import yaml

from .decode_pool import DecodePool, TileShapeError, read_tile, tile_header_shape
from .gpkg import GpkgWriter
from .shard import run_sharded, shard_range
from .spec import BATCHED_NMS_HELP, load_d2_yaml
from .vectorize import instances_to_features, instances_to_gpkg_rows
from .weights import infer_num_classes, load_checkpoint, synthetic_weights

SECTION = "make_detections.py"
log = logging.getLogger("make_detections")


def tile_extent(meta: Dict[str, Any], file_name: str) -> Tuple[Optional[Sequence[float]], Optional[int]]:
    """Georeference of one tile from ``img_metadata.json`` (R:config/config_obj_detec.yaml:78): returns
    ((xmin, ymin, xmax, ymax), epsg) or (None, None).  Keys are matched by path or basename; the extent may be
    stored as ``extent``/``bbox`` [xmin, ymin, xmax, ymax] or as west/south/east/north."""
    rec = meta.get(file_name) or meta.get(os.path.basename(file_name))
    if rec is None:
        for k, v in meta.items():
            if os.path.basename(k) == os.path.basename(file_name):
                rec = v
                break
    if not isinstance(rec, dict):
        return None, None
    ext = rec.get("extent") or rec.get("bbox")
    if isinstance(ext, dict):
        ext = [ext.get("xmin"), ext.get("ymin"), ext.get("xmax"), ext.get("ymax")]
    if ext is None and all(k in rec for k in ("west", "south", "east", "north")):
        ext = [rec["west"], rec["south"], rec["east"], rec["north"]]
    epsg = None
    for k in ("crs", "srs", "epsg"):
        if k in rec:
            s = str(rec[k])
            digits = "".join(ch for ch in s.split(":")[-1] if ch.isdigit())
            epsg = int(digits) if digits else None
            break
    return (list(map(float, ext)) if ext is not None else None), epsg


def _close_pools(pools: Dict[Tuple[int, ...], DecodePool]) -> None:
    """Unpin every decode slab BEFORE its shared memory goes away (a registered range that outlives its mapping would let a later
    array at a recycled address pass for pinned -- engine.Engine.upload_async), then stop the workers.  Error and normal path."""
    from .engine import unregister_host_buffer
    for pl in pools.values():
        try:
            if pl.slab is not None:
                unregister_host_buffer(pl.slab)
        finally:
            pl.close()
    pools.clear()


def road_labels(coco: Dict[str, Any], dataset: str = "") -> Dict[Any, Tuple[List[Any], List[List[np.ndarray]]]]:
    """The road labels of a COCO file for ``--road-votes``: image id -> (road ids, labels), one label per polygon annotation in the
    file's order, a label being the list of its rings ([x0, y0, x1, y1, ...], tile pixels).  The road is the annotation's ``road_id``
    where present, else its ``id``.  Crowd and RLE annotations, and rings of fewer than three points, are skipped with a log line."""
    out: Dict[Any, Tuple[List[Any], List[List[np.ndarray]]]] = {}
    skipped = 0
    for a in coco.get("annotations", []):
        seg = a.get("segmentation")
        if a.get("iscrowd") or not isinstance(seg, list):
            skipped += 1
            continue
        rings = [np.asarray(r, np.float64).reshape(-1) for r in seg if len(r) >= 6 and len(r) % 2 == 0]
        if not rings:
            skipped += 1
            continue
        ids, labs = out.setdefault(a["image_id"], ([], []))
        ids.append(a.get("road_id", a.get("id")))
        labs.append(rings)
    if skipped:
        log.info("%s: %d annotation(s) are crowd regions, RLE masks or have no polygon: they are no road labels", dataset, skipped)
    return out


def road_covers(coco: Dict[str, Any]) -> Dict[Any, str]:
    """For ``--road-stats``: road -> the category name of its first label (the annotations ``road_labels`` takes, in the file's order).
    Empty where the file names no categories: then no per-cover table is written."""
    names = {c["id"]: c.get("name") for c in coco.get("categories", []) if c.get("name")}
    out: Dict[Any, str] = {}
    for a in coco.get("annotations", []):
        seg = a.get("segmentation")
        if a.get("iscrowd") or not isinstance(seg, list) or not any(len(r) >= 6 and len(r) % 2 == 0 for r in seg):
            continue
        if a.get("category_id") in names:
            out.setdefault(a.get("road_id", a.get("id")), names[a["category_id"]])
    return out


def thr_tag(thr: float) -> str:
    return str(thr).replace(".", "dot")


def host_pool_sizes(host_workers: Optional[int], decode_procs: Optional[int], vector_threads: Optional[int],
                    cores: Optional[int] = None, local_world: Optional[int] = None) -> Tuple[int, int, int, int]:
    """Sizes of the three host pools of one rank.  Measured on a one-GPU box (16 cores for the rank): 4 decode processes + 4 host threads + 4
    vectoriser threads feed one MI355X at 1 880 tiles/s with the forward thread waiting 0.2 ms per batch for input.
    With N ranks on one host every rank gets cores / N of them (``LOCAL_WORLD_SIZE`` from torchrun); below 16 cores per rank the
    defaults shrink proportionally (a quarter of the share each, at least 1) so that 8 ranks never oversubscribe a small host.
    Values given on the command line are kept."""
    if cores is None:
        try:
            cores = len(os.sched_getaffinity(0))
        except AttributeError:
            cores = os.cpu_count() or 1
    if local_world is None:
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1)
    share = max(1, cores // max(1, local_world))
    auto = min(4, max(1, share // 4))
    hw = auto if host_workers is None else host_workers
    return hw, (auto if decode_procs is None else decode_procs), (auto if vector_threads is None else vector_threads), share


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("config_file", help="YAML with a 'make_detections.py' section (R:config/config_obj_detec.yaml)")
    ap.add_argument("--batch", type=int, default=16, help="tiles per engine call")
    ap.add_argument("--lanes", type=int, default=2, help="engine contexts fed alternately, each on its own stream (engine.LanePipeline); 2 keeps the GPU busy while the host collects a batch")
    ap.add_argument("--synthetic-weights", action="store_true",
                    help="use seeded synthetic weights instead of model_weights.pth_file (demo / smoke tests)")
    ap.add_argument("--host-workers", type=int, default=None,
                    help="threads for tile decode / vectorisation around the GPU call (default: 4, fewer when this rank's share of the host's cores is under 16)")
    ap.add_argument("--decode-procs", type=int, default=None,
                    help="worker PROCESSES that decode tiles into shared memory (decode_pool.DecodePool); 0 = decode on the --host-workers threads (default: as --host-workers)")
    ap.add_argument("--vector-threads", type=int, default=None, help="threads inside one rs_vectorize_masks call (default: as --host-workers)")
    ap.add_argument("--vectorize", choices=("host", "device"), default="host",
                    help="where detection masks become polygons: 'host' = csrc/vectorize.cpp on the vectoriser threads (masks cross PCIe as crops); "
                         "'device' = csrc/polygonize.hip behind the forward, only polygon tables come back, and only instances beyond the kernel's "
                         "capacities are vectorised on the host (same polygons either way; DESIGN.md 3.7)")
    ap.add_argument("--precision", choices=("fp16", "split", "fp32"), default="fp16",
                    help="fp16: fp16 operands / fp32 accumulate on the matrix cores (fastest; meets the SURVEY 8d tolerance on a trained detector); "
                         "split: the reference's fp32 results on the fp16 matrix cores -- every operand as hi + lo fp16 planes, three products, about 2.7x "
                         "slower than fp16 (DESIGN.md section 3.1d); fp32: fp32 activations and weights on the fp32 matrix cores, about 7x slower (section 3.1c)")
    ap.add_argument("--geojson", action="store_true", help="also write <dataset>_detections_..._threshold.geojson (slow: Python feature dicts)")
    ap.add_argument("--tagged-samples", type=int, default=10,
                    help="tagged preview PNGs per dataset in sample_tagged_img_subfolder (0 = none)")
    ap.add_argument("--max-tiles", type=int, default=0, help="debug: only the first N tiles of every dataset")
    ap.add_argument("--batched-nms", choices=("per-category", "torchvision"), default="per-category", help=BATCHED_NMS_HELP)
    ap.add_argument("--road-votes", action="store_true",
                    help="also write <dataset>_road_votes.json, the cover class per road (raster_vote.reduce_votes): the polygon annotations of the "
                         "dataset's COCO file are the road labels of their tile (tile pixels; 'road_id' where present, else 'id'), counted against "
                         "the detection masks on the GPU behind every batch's forward (csrc/road_vote.h); a batch beyond the device pool is voted "
                         "on the host from its masks.  Needs datasets of one tile shape.  Every other output is unchanged")
    ap.add_argument("--road-stats", action="store_true",
                    help="also write <dataset>_road_stats.json, the band statistics per road of the reference's statistical route (band_stats.py: "
                         "min, max, median, mean, count, std and margin per road and band, and per cover type where the annotations carry a "
                         "category): the road labels of --road-votes (which it does not need), their pixels counted into histograms on the GPU "
                         "behind every batch's forward (csrc/band_hist.h); a batch beyond the device pool is counted on the host.  Needs "
                         "datasets of one tile shape.  Every other output is unchanged")
    ap.add_argument("--road-metrics", action="store_true",
                    help="after the last dataset also write road_metrics.json, the reference's final metrics (road_metrics.py: the balanced F1 of "
                         "the per-road cover classes at the best score threshold, per dataset and zone, accuracy, the sweep on the difference of "
                         "indices, the baseline): the road labels of --road-votes (which it does not need) and their categories, the vote of "
                         "every threshold formed in one pass on the GPU behind every batch's forward (csrc/road_vote.h, the sweep).  Needs "
                         "categories in the COCO files and datasets of one tile shape.  Every other output is unchanged")
    ap.add_argument("--metric-thresholds", default=None,
                    help="comma-separated score thresholds of --road-metrics, at most 32 (31 together with --road-votes); default: "
                         "np.arange(0, 1., 0.05), the reference's 20")
    ap.add_argument("--vote-geometry", choices=("pixels", "polygons"), default="pixels",
                    help="what the weight of a (road, detection) pair of --road-votes / --road-metrics is measured on: 'pixels' = counts on the tile "
                         "grid against the masks; 'polygons' = the area of the polygon intersection of the label's rings with the detection polygons "
                         "that go into the GeoPackage (after RDP), as the reference's overlay (csrc/poly_overlap.h).  Needs --vectorize device; a "
                         "label's rings are taken as disjoint exteriors.  The JSON files then carry \"geometry\": \"polygons\"")
    ap.add_argument("--vote-threshold", type=float, default=None,
                    help="score a detection needs to vote (default: 'threshold' of the YAML's 'determine_class.py' section where it exists, else 0)")
    return ap


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s", stream=sys.stderr)
    args.host_workers, args.decode_procs, args.vector_threads, share = host_pool_sizes(args.host_workers, args.decode_procs, args.vector_threads)
    logging.getLogger("make_detections").info("host pools of this rank: %d decode processes, %d host threads, %d vectoriser threads (%d cores for the rank)",
                                              args.decode_procs, args.host_workers, args.vector_threads, share)

    if args.vote_geometry == "polygons":             # refused up front, before a file is read or a device touched
        if args.vectorize != "device":
            raise SystemExit("--vote-geometry polygons reads the device polygoniser's vertex tables: it needs --vectorize device")
        if not (args.road_votes or args.road_metrics):
            raise SystemExit("--vote-geometry polygons serves --road-votes / --road-metrics: name one of them")
    with open(args.config_file) as f:
        whole_cfg = yaml.safe_load(f)
    cfg = whole_cfg[SECTION]
    vote_thr = float(args.vote_threshold if args.vote_threshold is not None else (whole_cfg.get("determine_class.py") or {}).get("threshold", 0))
    votes: Dict[str, Any] = {"labels": None, "by_file": {}}      # --road-votes / --road-stats: the running dataset's labels per batch, its vote tables per tile
    band_by_file: Dict[str, Any] = {}                            # --road-stats: the running dataset's histograms per tile
    sweep_by_file: Dict[str, Any] = {}                           # --road-metrics: the running dataset's sweep tables per tile
    metric_sets: Dict[str, Any] = {}                             # --road-metrics, rank 0: dataset -> (road ids per tile, sweep tables per tile)
    metric_batches = {"host": 0, "of": 0}
    metric_thr = None
    if args.road_metrics:
        from .road_metrics import REFERENCE_THRESHOLDS
        try:
            metric_thr = (np.asarray([float(v) for v in args.metric_thresholds.split(",")], np.float64) if args.metric_thresholds
                          else REFERENCE_THRESHOLDS)
        except ValueError:
            raise SystemExit(f"--metric-thresholds: {args.metric_thresholds!r} is not a comma-separated list of numbers")
        most = 31 if args.road_votes else 32
        if not 1 <= metric_thr.size <= most or not np.isfinite(metric_thr).all():
            raise SystemExit(f"--road-metrics takes 1 to {most} finite thresholds{' with --road-votes' if args.road_votes else ''}, got {metric_thr.size}")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=os.environ.get("RS_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
        import torch
        local_rank = local_rank % max(1, torch.cuda.device_count())      # several ranks may share a card (tests on a one-GPU box); counting devices does not initialise the GPU
        logging.getLogger("make_detections").info("rank %d of %d ranks on device %d", rank, world, local_rank)

    os.chdir(cfg["working_directory"])
    os.makedirs(cfg.get("log_subfolder", "logs"), exist_ok=True)
    meta: Dict[str, Any] = {}
    if cfg.get("image_metadata_json") and os.path.exists(cfg["image_metadata_json"]):
        with open(cfg["image_metadata_json"]) as f:
            meta = json.load(f)
    coco = {}
    for name, path in cfg["COCO_files"].items():
        with open(path) as f:
            coco[name] = json.load(f)
    cats = sorted({c["id"] for d in coco.values() for c in d.get("categories", [])})
    if args.road_metrics and not all(any(c.get("name") for c in d.get("categories", [])) for d in coco.values()):
        raise SystemExit("--road-metrics needs the categories of the road labels: a COCO file names none")
    thr = float(cfg.get("score_lower_threshold", 0.05))
    rdp_cfg = cfg.get("rdp_simplification", {}) or {}

    if args.synthetic_weights:
        spec = load_d2_yaml(cfg["detectron2_config_file"], num_classes=max(len(cats), 1)).replace(score_thresh_test=thr)
        W = synthetic_weights(spec, seed=0)
    else:
        W = load_checkpoint(cfg["model_weights"]["pth_file"])
        k = infer_num_classes(W)
        if cats and len(cats) != k:
            raise SystemExit(f"checkpoint has {k} classes but the COCO files define {len(cats)} categories")
        spec = load_d2_yaml(cfg["detectron2_config_file"], num_classes=k).replace(score_thresh_test=thr)

    if args.precision != spec.precision:
        spec = spec.replace(precision=args.precision)
        log.info("inference in %s", {"fp32": "reference precision (fp32 on the matrix cores)", "split": "reference-equivalent precision (hi + lo fp16 operand planes, three products)",
                                     "fp16": "fp16 operands / fp32 accumulate"}[args.precision])
    spec = spec.replace(batched_nms=args.batched_nms.replace("-", "_"))
    log.info("batched_nms: %s", {"per_category": "per-category (one NMS per FPN level / class)",
                                 "torchvision": "torchvision (size rule: shifted coordinates at <= 1000 boxes per image)"}[spec.batched_nms])
    from .engine import Predictor      # fails loudly without librs_engine.so / a HIP device
    # saturation (activations clamped to the fp16 range) is reported once per dataset below, not per batch
    # the epsilon the device polygoniser simplifies with is the YAML's, as on the host path (rdp_simplification: enabled / epsilon)
    dev_eps = float(rdp_cfg.get("epsilon", 0.75)) if bool(rdp_cfg.get("enabled", False)) else 0.0
    pred_kw = dict(max_batch=args.batch, device=local_rank, lanes=args.lanes, on_saturation="ignore", vectorize=args.vectorize, rdp_epsilon=dev_eps)
    if args.vectorize == "device":
        # polygons come back with the detections; the tagged previews below run their own forward (Predictor.__call__), which always
        # returns masks, so no streamed batch has to bring masks along.  No vectoriser pool: the few instances the kernel leaves to
        # the host are traced on the thread that finishes their batch.
        args.vector_threads = 1
        log.info("polygons on the device (rdp epsilon %s); the vectoriser threads are not started", dev_eps if dev_eps > 0 else "off")
    predictor = Predictor(spec, W, **pred_kw)
    fell_back = {"instances": 0, "of": 0}          # device mode: instances the polygoniser left to the host vectoriser

    class _Batch(list):       # one batch's results with the saturation counts of its forward, for finish()
        saturation: Dict[str, int] = {}

    def with_saturation(out: List[Any]) -> "_Batch":
        b = _Batch(out)
        b.saturation = dict(predictor.last_saturation)
        return b

    saturated: List[Tuple[str, Dict[str, int]]] = []      # (first tile of the batch, counts) of every batch that saturated

    # decode (PIL), GPU forward and vectorisation (C++, rs_vectorize_masks) overlap across batches (shard.run_sharded)
    busy = {"decode": 0.0, "predict": 0.0, "vectorise": 0.0}      # seconds summed over the threads that ran each stage

    def prepare(entries: Sequence[dict]) -> List[Any]:
        t = time.perf_counter()
        out = [read_tile(e["file_name"]) for e in entries]
        busy["decode"] += time.perf_counter() - t
        return out

    def predict_batch(ims: Sequence[Any]) -> List[Any]:
        t = time.perf_counter()
        out = predictor.predict_batch(ims)
        busy["predict"] += time.perf_counter() - t
        return with_saturation(out)

    def predict_stream(batches):
        # the whole dataset through one lane pipeline: batch k+1 uploads and runs while batch k's results come back
        if votes["labels"] is None:
            it = predictor.predict_stream(batches)
        else:
            it = predictor.predict_stream(batches, labels=iter(votes["labels"]), vote_threshold=vote_thr, band_stats=args.road_stats,
                                          road_votes=args.road_votes, vote_sweep=metric_thr, vote_geometry=args.vote_geometry)
        while True:
            t = time.perf_counter()
            out = next(it, None)
            busy["predict"] += time.perf_counter() - t
            if out is None:
                return
            yield with_saturation(out)

    def finish(entries: Sequence[dict], outs: List[Any]) -> List[Any]:
        # per tile: (GeoPackage rows, bbox[, GeoJSON features]) -- masks -> polygons -> RDP -> georeferenced blobs in C++
        t_fin = time.perf_counter()
        if getattr(outs, "saturation", None) and entries:
            saturated.append((entries[0]["file_name"], outs.saturation))
        res = []
        for e, o in zip(entries, outs):
            ext, epsg_t = tile_extent(meta, e["file_name"])
            name = os.path.basename(e["file_name"])
            rdp_on, eps = bool(rdp_cfg.get("enabled", False)), float(rdp_cfg.get("epsilon", 0.75))
            if votes["labels"] is not None and args.road_votes:
                votes["by_file"][e["file_name"]] = o["instances"].road_votes
            if votes["labels"] is not None and args.road_stats:
                band_by_file[e["file_name"]] = o["instances"].band_hist
            if votes["labels"] is not None and args.road_metrics:
                sweep_by_file[e["file_name"]] = o["instances"].road_vote_sweep
            carried = getattr(o["instances"], "_polygons", None)
            if carried is not None:
                fell_back["instances"] += int(len(carried.flagged))
                fell_back["of"] += len(o["instances"])
            rows, bbox = instances_to_gpkg_rows(o["instances"], name, ext, rdp_on, eps, srs_id=cur_srs["id"], threads=args.vector_threads)
            feats = instances_to_features(o["instances"], name, ext, rdp_on, eps, threads=args.vector_threads) if args.geojson else None
            res.append((rows, bbox, feats))
        busy["vectorise"] += time.perf_counter() - t_fin
        return res

    cur_srs = {"id": -1}
    pools: Dict[Tuple[int, ...], DecodePool] = {}       # process decoders by tile shape (spawned once, reused by every dataset of that shape)
    for dataset, d in coco.items():
        images = d.get("images", [])
        if args.max_tiles:
            images = images[: args.max_tiles]
        t0 = time.time()
        epsg = None
        for e in images:
            _, epsg = tile_extent(meta, e["file_name"])
            if epsg:
                break
        cur_srs["id"] = int(epsg) if epsg else -1
        source = None
        # The process decoder serves ONE tile shape per dataset (its slab is a fixed (n, H, W, C) array); the thread path groups runs of
        # equal shape as the reference's per-tile cv2.imread loop effectively does.  Decide before starting: COCO width/height when every
        # entry carries them, the file headers otherwise; a dataset of mixed shapes keeps the thread path.
        if args.decode_procs > 0 and images:
            shape = tuple(read_tile(images[0]["file_name"]).shape)
            if all("width" in e and "height" in e for e in images):
                uniform = all((int(e["height"]), int(e["width"])) == shape[:2] for e in images)
            else:
                uniform = all(tile_header_shape(e["file_name"]) == shape for e in images)
            if not uniform:
                log.info("%s: tiles of several shapes -- decoding on the %d host threads instead of the process decoder", dataset, args.host_workers)
            elif shape not in pools:
                from .engine import register_host_buffer
                pools[shape] = DecodePool(args.decode_procs, args.batch, shape, spare=predictor.lanes + 2)
                if not register_host_buffer(pools[shape].slab):      # pinned: batches go from the slab to the device without a staging copy
                    log.info("the decode slab could not be pinned; batches are staged through the engine's own pinned buffer")
            pool = pools.get(shape) if uniform else None
            if uniform:
                t_p = time.time()
                predictor.prepare(shape)                # engines built + kernels loaded while the decoder processes start
                log.info("%s: lane pipeline for %s tiles ready in %.2f s", dataset, shape, time.time() - t_p)

            def pool_source(chunks, pool=pool):
                it = pool.batches(chunks, key=lambda e: os.path.abspath(e["file_name"]))
                while True:
                    t = time.perf_counter()
                    b = next(it, None)
                    busy["decode"] += time.perf_counter() - t          # here: time the forward thread WAITED for decoded tiles
                    if b is None:
                        return
                    yield b
            source = pool_source if pool is not None else None
        if args.road_votes or args.road_stats or args.road_metrics:
            lo, hi = shard_range(len(images), rank, world)
            by_image = road_labels(d, dataset)
            votes["by_file"] = {}
            band_by_file.clear()
            sweep_by_file.clear()
            votes["labels"] = [[by_image.get(e["id"], ([], []))[1] for e in images[i:min(i + args.batch, hi)]] for i in range(lo, hi, args.batch)]
        try:
            try:
                per_tile = run_sharded(images, predict_batch, args.batch, rank, world, gather=False, prepare=prepare, finish=finish,
                                       workers=args.host_workers, predict_stream=predict_stream, prepared_source=source)
            except TileShapeError as ex:
                # the COCO sizes (or the band count of the first tile) did not hold for every file: this dataset again on the thread path
                log.warning("%s: %s -- running the dataset again with thread decoding", dataset, ex)
                predictor.close()
                saturated.clear()
                predictor = Predictor(spec, W, **pred_kw)
                fell_back.update(instances=0, of=0)
                per_tile = run_sharded(images, predict_batch, args.batch, rank, world, gather=False, prepare=prepare, finish=finish,
                                       workers=args.host_workers, predict_stream=predict_stream, prepared_source=None)
        except BaseException:
            _close_pools(pools)
            raise
        if saturated:
            order = {e["file_name"]: i for i, e in enumerate(images)}
            total: Dict[str, int] = {}
            for _, sat in saturated:
                for k, v in sat.items():
                    total[k] = total.get(k, 0) + v
            first = min((f for f, _ in saturated), key=lambda f: order.get(f, len(order)))
            top = ", ".join(f"{k} {v}" for k, v in sorted(total.items(), key=lambda kv: -kv[1])[:3])
            log.warning("%s: %d batch(es) had activations clamped to the fp16 range (first affected batch starts at tile %s); largest counts: %s "
                        "-- detections of those batches may be wrong, --precision fp32 never clamps", dataset, len(saturated),
                        os.path.basename(first), top)
            saturated.clear()
        if args.road_votes:
            # every rank's per-(tile, label) tables travel to rank 0, which reduces them in global tile order: the file does not depend
            # on the world size
            mine = [(by_image.get(e["id"], ([], []))[0], votes["by_file"][e["file_name"]][:3]) for e in images[lo:hi]]
            parts: List[Any] = [(mine, predictor.vote_fallbacks)]
            if world > 1:
                import torch.distributed as dist
                parts = [None] * world if rank == 0 else None
                dist.gather_object((mine, predictor.vote_fallbacks), parts, dst=0)
            if rank == 0:
                from .raster_vote import CLASS_NAMES, reduce_votes
                rows = [t for part, _ in parts for t in part]             # rank order == tile order for contiguous blocks
                K = spec.num_classes
                by_id = {c["id"]: c.get("name") for c in d.get("categories", [])}
                names = {i: by_id.get(cid) for i, cid in enumerate(cats)}
                if len(names) != K or not all(names.values()):
                    names = dict(CLASS_NAMES) if K == len(CLASS_NAMES) else {i: str(i) for i in range(K)}
                table = reduce_votes([t for _, t in rows], [ids for ids, _ in rows], names)
                with open(f"{dataset}_road_votes.json", "w") as f:
                    f.write(json.dumps(table if args.vote_geometry == "pixels" else {"geometry": args.vote_geometry, "roads": table}))
                log.info("%s: %d road labels on %d tiles -> %d roads in %s_road_votes.json (vote threshold %g); %d of %d batches were voted on the host",
                         dataset, sum(len(ids) for ids, _ in rows), len(rows), len(table), dataset, vote_thr, sum(fb for _, fb in parts),
                         sum(len(range(*shard_range(len(images), r, world), args.batch)) for r in range(world)))
        if args.road_stats:
            # every rank sums its own tiles' histograms per road; the per-road sums travel to rank 0, which adds them in rank order =
            # tile order.  Integer sums: the file does not depend on the world size
            from . import band_stats
            mine_h = band_stats.reduce_band_hist([band_by_file[e["file_name"]] for e in images[lo:hi]],
                                                 [by_image.get(e["id"], ([], []))[0] for e in images[lo:hi]])
            parts_h: List[Any] = [(mine_h, predictor.band_fallbacks)]
            if world > 1:
                import torch.distributed as dist
                parts_h = [None] * world if rank == 0 else None
                dist.gather_object((mine_h, predictor.band_fallbacks), parts_h, dst=0)
            if rank == 0:
                by_road: Dict[Any, Any] = {}
                for part, _ in parts_h:
                    for rid, h in part.items():
                        by_road[rid] = by_road[rid] + h if rid in by_road else h
                doc: Dict[str, Any] = {"columns": list(band_stats.COLUMNS),
                                       "roads": [{"road_id": rid, "bands": band_stats.json_rows(band_stats.stats_from_hist(h))} for rid, h in by_road.items()]}
                covers = road_covers(d)
                if covers:
                    doc["covers"] = [{"cover_type": c, "bands": band_stats.json_rows(rows)} for c, rows in band_stats.cover_stats(by_road, covers).items()]
                with open(f"{dataset}_road_stats.json", "w") as f:
                    f.write(json.dumps(doc))
                log.info("%s: band statistics of %d roads%s in %s_road_stats.json; %d of %d batches were counted on the host", dataset, len(by_road),
                         f" and {len(doc['covers'])} cover types" if covers else "", dataset, sum(fb for _, fb in parts_h),
                         sum(len(range(*shard_range(len(images), r, world), args.batch)) for r in range(world)))
        if args.road_metrics:
            # as --road-votes: every rank's per-(tile, label) tables of every threshold travel to rank 0 in tile order, which keeps them
            # until the last dataset: the file does not depend on the world size
            mine_s = [(by_image.get(e["id"], ([], []))[0], sweep_by_file[e["file_name"]][:3]) for e in images[lo:hi]]
            parts_s: List[Any] = [(mine_s, predictor.vote_fallbacks)]
            if world > 1:
                import torch.distributed as dist
                parts_s = [None] * world if rank == 0 else None
                dist.gather_object((mine_s, predictor.vote_fallbacks), parts_s, dst=0)
            if rank == 0:
                rows_s = [t for part, _ in parts_s for t in part]
                metric_sets[dataset] = ([ids for ids, _ in rows_s], [t for _, t in rows_s], road_covers(d))
                metric_batches["host"] += sum(fb for _, fb in parts_s)
                metric_batches["of"] += sum(len(range(*shard_range(len(images), r, world), args.batch)) for r in range(world))
        votes["labels"] = None
        # Every rank writes the rows of ITS block of tiles into its own GeoPackage shard (rank 0: the output file itself); rank 0 then appends the
        # other ranks' shards in rank order = tile order with SQLite ATTACH -- no row travels between processes ("each rank ...
        # its own output shard; host merges shards into one GeoPackage per dataset").  The ranks of one node share the working directory.
        base = f"{dataset}_detections_at_{thr_tag(thr)}_threshold"
        t_w = time.time()
        shard_path = base + ".gpkg" if rank == 0 else f"{base}.rank{rank}.gpkg"
        if rank != 0 and os.path.exists(shard_path):
            os.remove(shard_path)
        gw = GpkgWriter(shard_path, table=base, epsg=epsg)
        for rows, bbox, _ in per_tile:
            gw.add_rows(rows, bbox)
        if args.geojson and world > 1:
            with open(f"{base}.rank{rank}.features.json", "w") as f:
                f.write(json.dumps([ft for _, _, fs in per_tile for ft in fs]))
        if rank != 0:
            gw.close()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()                                   # every shard is complete on disk
        if rank != 0:
            continue
        for r in range(1, world):
            sp = f"{base}.rank{r}.gpkg"
            gw.append_shard(sp)
            os.remove(sp)
        n = gw.close()
        dt_write = time.time() - t_w
        if args.geojson:
            feats = [f for _, _, fs in per_tile for f in fs]
            for r in range(world if world > 1 else 0):
                fp = f"{base}.rank{r}.features.json"
                if r > 0:
                    with open(fp) as f:
                        feats += json.load(f)
                os.remove(fp)
            with open(base + ".geojson", "w") as f:
                f.write(json.dumps({"type": "FeatureCollection", "features": feats}))   # dumps() = C encoder; dump() streams through the slow Python one
        dt = time.time() - t0
        if args.vectorize == "device":
            log.info("%s: %d tiles -> %d features in %.1f s (%.1f tiles/s) -> %s.gpkg; %d of %d instances fell back to the host vectoriser",
                     dataset, len(images), n, dt, len(images) / max(dt, 1e-9), base, fell_back["instances"], fell_back["of"])
            fell_back.update(instances=0, of=0)
        else:
            log.info("%s: %d tiles -> %d features in %.1f s (%.1f tiles/s) -> %s.gpkg", dataset, len(images), n, dt,
                     len(images) / max(dt, 1e-9), base)
        log.info("%s: stage busy time (summed over threads) decode %.2f s, predict %.2f s, vectorise %.2f s, write %.2f s",
                 dataset, busy["decode"], busy["predict"], busy["vectorise"], dt_write)
        for shp, pl in getattr(predictor, "_pipes", {}).items():
            tm = getattr(pl, "timing", None)
            if tm and tm["batches"]:
                log.info("%s: forward thread per batch of %s tiles: wait for input %.2f ms, wait for results %.2f, upload %.2f, enqueue %.2f, collect %.2f (%d batches)",
                         dataset, shp, *(1e3 * tm[k] / tm["batches"] for k in ("pull", "wait_results", "upload", "enqueue", "collect")), tm["batches"])
        busy.update({k: 0.0 for k in busy})
        sub = cfg.get("sample_tagged_img_subfolder")
        if sub and args.tagged_samples > 0:
            # the reference tags the first images of every dataset with their predictions (R:config/config_obj_detec.yaml:77)
            from .tagging import draw_instances
            os.makedirs(sub, exist_ok=True)
            names = [c["name"] for c in sorted(d.get("categories", []), key=lambda c: c["id"])]
            for e in images[: args.tagged_samples]:
                im = read_tile(e["file_name"])
                inst = predictor(im)["instances"]
                rgb = im[:, :, ::-1][:, :, :3]              # read_tile hands the file's bands over in reverse (cv2) order
                png = os.path.join(sub, f"{dataset}_det_{os.path.splitext(os.path.basename(e['file_name']))[0]}.png")
                draw_instances(rgb, inst.pred_boxes, inst.pred_classes, inst.scores, inst.pred_masks, names or None).save(png)
            log.info("%s: %d tagged sample images -> %s/", dataset, min(len(images), args.tagged_samples), sub)
    if args.road_metrics and rank == 0:
        from . import road_metrics
        from .raster_vote import CLASS_NAMES
        K = spec.num_classes
        by_id = {c["id"]: c.get("name") for d in coco.values() for c in d.get("categories", [])}
        names = {i: by_id.get(cid) for i, cid in enumerate(cats)}
        if len(names) != K or not all(names.values()):
            names = dict(CLASS_NAMES) if K == len(CLASS_NAMES) else {i: str(i) for i in range(K)}
        classes = [names[i] for i in range(K)]
        categories: Dict[Any, str] = {}
        for _, _, covers in metric_sets.values():            # a road's category: its first label's, in dataset order
            for rid, c in covers.items():
                categories.setdefault(rid, c)
        asked = str((whole_cfg.get("final_metrics.py") or {}).get("baseline", ""))
        base_cls = next((c for c in classes if c in asked), "artificial")
        doc = road_metrics.report({k: v[:2] for k, v in metric_sets.items()}, categories, classes, metric_thr, names, base_cls)
        if args.vote_geometry != "pixels":
            doc["geometry"] = args.vote_geometry
        with open("road_metrics.json", "w") as f:
            f.write(json.dumps(doc))
        log.info("road metrics: %d thresholds on %d roads of %d datasets -> best threshold %g (balanced f1 %.4f on %s) in road_metrics.json; "
                 "%d of %d batches were voted on the host", len(doc["thresholds"]), len(categories), len(metric_sets), doc["best_threshold"],
                 doc["sweep"][doc["best_index"]]["global"]["f1b"], doc["sweep_on"], metric_batches["host"], metric_batches["of"])
    _close_pools(pools)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
