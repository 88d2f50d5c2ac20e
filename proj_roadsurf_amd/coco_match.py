"""COCOeval's ``evaluateImg`` as the library runs it (csrc/coco_match.h): ``rs_host_coco_match`` on host arrays and ``rs_op_coco_match``
on the GPU (arrays uploaded through torch), both returning the five match tables of include/rs_engine.h, and the step from the tables
to the records of ``coco_eval.match_images``.  A batch is a dict of arrays:

    det_boxes (n, D, 4) float32, det_scores (n, D) float32, det_classes (n, D) int32, det_count (n,) int32   -- as ``rs_dets``
    gt_boxes (I, 4) float64 XYXY, gt_classes (I,) int32, tile_first (n + 1,) int32                            -- tile t owns I[t] .. I[t+1]
    inter (n, D, cap) int32, det_area (n, D) int32, gt_area (n, cap) int32                                    -- ``rs_op_mask_pair_counts``
    num_classes

Crowd regions and annotated areas are not modelled: ``Engine.eval_matches`` sends such a batch to the host."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from . import coco_eval

TABLES = ("order", "class_first", "gt_per_class", "matched", "ignored", "npig")
MAX_SLOTS = 1024       # CM_MAX_SLOTS


def empty_tables(n: int, D: int, K: int, prefill: int = 0) -> Dict[str, np.ndarray]:
    W, T, A = (D + 31) // 32, len(coco_eval.IOU_THRS), len(coco_eval.AREA_RNG)
    shapes = {"order": (n, D), "class_first": (n, K + 1), "gt_per_class": (n, K), "matched": (n, 2, A, T, W), "ignored": (n, 2, A, T, W),
              "npig": (n, 2, A, K)}
    return {k: np.full(s, prefill, np.int32).view(np.uint32 if k in ("matched", "ignored") else np.int32) for k, s in shapes.items()}


def _inputs(b: Dict) -> List[np.ndarray]:
    n, D = b["det_scores"].shape
    I = int(b["tile_first"][-1])
    return [np.ascontiguousarray(b["det_boxes"], np.float32).reshape(n, D, 4), np.ascontiguousarray(b["det_scores"], np.float32),
            np.ascontiguousarray(b["det_classes"], np.int32), np.ascontiguousarray(b["det_count"], np.int32),
            np.ascontiguousarray(np.concatenate([np.asarray(b["gt_boxes"], np.float64).reshape(I, 4), np.zeros((1, 4))])),     # never empty
            np.ascontiguousarray(np.concatenate([np.asarray(b["gt_classes"], np.int32).reshape(I), np.zeros(1, np.int32)])),
            np.ascontiguousarray(b["tile_first"], np.int32), np.ascontiguousarray(b["inter"], np.int32),
            np.ascontiguousarray(b["det_area"], np.int32), np.ascontiguousarray(b["gt_area"], np.int32)]


def host_tables(b: Dict) -> Dict[str, np.ndarray]:
    """``rs_host_coco_match`` on a batch: no GPU."""
    from .engine import _check, load_library
    lib = load_library()
    arrs = _inputs(b)
    n, D = arrs[1].shape
    cap, K = int(arrs[7].shape[2]), int(b["num_classes"])
    out = empty_tables(n, D, K, prefill=-7)          # every entry is written
    thr = np.ascontiguousarray(coco_eval.IOU_THRS, np.float64)
    _check(lib, lib.rs_host_coco_match(*[a.ctypes.data for a in arrs], thr.ctypes.data, n, K, D, cap, *[out[k].ctypes.data for k in TABLES]),
           "rs_host_coco_match")
    return out


def device_tables(b: Dict, prefill: int = -7) -> Dict[str, np.ndarray]:
    """``rs_op_coco_match`` on a batch, uploaded and read back through torch.  ``prefill``: what the output buffers hold before."""
    import torch
    from .engine import _check, load_library
    lib = load_library()
    arrs = _inputs(b)
    n, D = arrs[1].shape
    cap, K = int(arrs[7].shape[2]), int(b["num_classes"])
    dev = torch.device("cuda")
    ins = [torch.from_numpy(a).to(dev) for a in arrs]
    host = empty_tables(n, D, K, prefill)
    outs = {k: torch.from_numpy(host[k].view(np.int32)).to(dev) for k in TABLES}
    thr = np.ascontiguousarray(coco_eval.IOU_THRS, np.float64)
    torch.cuda.synchronize()
    _check(lib, lib.rs_op_coco_match(*[t.data_ptr() for t in ins], thr.ctypes.data, n, K, D, cap, *[outs[k].data_ptr() for k in TABLES], None),
           "rs_op_coco_match")
    torch.cuda.synchronize()
    return {k: outs[k].cpu().numpy().view(host[k].dtype) for k in TABLES}


def records(b: Dict, tables: Dict[str, np.ndarray], iou_type: str) -> List[Dict]:
    """One ``match_images`` record per tile out of the tables."""
    return [coco_eval.records_from_tables(np.asarray(b["det_scores"])[t], *[tables[k][t] for k in TABLES], iou_type=iou_type)
            for t in range(len(b["det_count"]))]


def images(b: Dict):
    """The batch as the (gts, dets) dict lists ``coco_eval.match_images`` takes, for bbox and segm (integer counts)."""
    gts, dts = [], []
    first = np.asarray(b["tile_first"])
    for t in range(len(b["det_count"])):
        c, g0, g1 = int(b["det_count"][t]), int(first[t]), int(first[t + 1])
        gts.append({"boxes": np.asarray(b["gt_boxes"], np.float64).reshape(-1, 4)[g0:g1], "classes": np.asarray(b["gt_classes"])[g0:g1],
                    "mask_area": np.asarray(b["gt_area"])[t, :g1 - g0]})
        dts.append({"boxes": np.asarray(b["det_boxes"])[t, :c], "classes": np.asarray(b["det_classes"])[t, :c], "scores": np.asarray(b["det_scores"])[t, :c],
                    "mask_inter": np.asarray(b["inter"])[t, :c, :g1 - g0], "mask_area": np.asarray(b["det_area"])[t, :c]})
    return gts, dts
