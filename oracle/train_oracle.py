"""ORACLE (test infrastructure only) -- CPU fp32 restatement of the detectron2 0.6 *training* forward of the
Mask R-CNN R50-FPN the reference fine-tunes through the STDL object-detector's ``train_model.py``
(R:README.md:77, R:config/config_obj_detec.yaml:62-72, R:config/detectron2_config_3bands.yaml): label assignment,
sampling, the five losses, and -- through torch autograd on the differentiable forward of ``maskrcnn_oracle`` -- the
gradients the HIP backward path is checked against.

PARITY UNPINNED, as for ``maskrcnn_oracle.py``: detectron2 / torchvision / pycocotools are absent offline and the
reference ships no tests or fixtures for this path.  Pins: the reference YAML constants, closed-form known-answer
tests, and the vectors of detectron2's own published unit tests quoted in tests/test_train_oracle.py
(``tests/modeling/test_matcher.py``).

Randomness: detectron2 subsamples anchors / proposals with ``torch.randperm``; no two implementations agree on that
stream, so every sampling function here takes a ``perm(n) -> LongTensor`` callable (default: ``torch.randperm`` with
a generator) and the parity tests feed the SAME chosen indices to the oracle and to the HIP kernels.

Only ``tests/`` may import this module.  ``R:<n>`` = R:config/detectron2_config_3bands.yaml:<n>.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import maskrcnn_oracle as O
from proj_roadsurf_amd.spec import EngineSpec

Tensor = torch.Tensor
Perm = Callable[[int], Tensor]


@dataclass(frozen=True)
class TrainSpec:
    """Training-only YAML values (R: line numbers in detectron2_config_3bands.yaml)."""
    rpn_iou_thresholds: Tuple[float, float] = (0.3, 0.7)         # R:241-243
    rpn_iou_labels: Tuple[int, int, int] = (0, -1, 1)            # R:237-240
    rpn_batch_size_per_image: int = 256                          # R:223
    rpn_positive_fraction: float = 0.5                           # R:246
    rpn_smooth_l1_beta: float = 0.0                              # R:251
    rpn_bbox_reg_weights: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0)   # R:224-228
    rpn_pre_nms_topk_train: int = 2000                           # R:250
    rpn_post_nms_topk_train: int = 1000                          # R:248
    roi_iou_threshold: float = 0.5                               # R:187-188
    roi_batch_size_per_image: int = 1024                         # R:178
    roi_positive_fraction: float = 0.25                          # R:192
    roi_proposal_append_gt: bool = True                          # R:193
    box_smooth_l1_beta: float = 0.0                              # R:175
    base_lr: float = 0.01                                        # R:269
    momentum: float = 0.9                                        # R:281
    weight_decay: float = 1e-4                                   # R:303
    warmup_factor: float = 0.001                                 # R:300
    warmup_iters: int = 200                                      # R:301
    gamma: float = 0.8                                           # R:277
    steps: Tuple[int, ...] = (3000, 4000, 5000, 5500, 6000, 6500, 7000, 7500, 8000, 8500, 9000, 9500, 10000, 10500, 11000, 11500)  # R:283-299
    max_iter: int = 12000                                        # R:280
    ims_per_batch: int = 8                                       # R:278


# =====================================================================================
# Boxes, matcher, sampling  [EXT d2: structures/boxes.py, modeling/matcher.py, modeling/sampling.py]
# =====================================================================================
def pairwise_iou(boxes1: Tensor, boxes2: Tensor) -> Tensor:
    """``pairwise_iou`` (M,4) x (N,4) -> (M,N): intersection / (area1 + area2 - intersection), 0 where empty."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    wh = torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])
    wh.clamp_(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area1[:, None] + area2 - inter), torch.zeros(1, dtype=inter.dtype))


def matcher(match_quality_matrix: Tensor, thresholds: Sequence[float], labels: Sequence[int],
            allow_low_quality_matches: bool) -> Tuple[Tensor, Tensor]:
    """``Matcher.__call__``: (M gt, N predictions) -> (matches (N,) int64, match_labels (N,) int8).
    Ties of the per-prediction argmax go to the lower gt index (torch CPU ``max``)."""
    th = [-float("inf")] + list(thresholds) + [float("inf")]
    n = match_quality_matrix.shape[1]
    if match_quality_matrix.numel() == 0:
        return torch.zeros(n, dtype=torch.int64), torch.full((n,), labels[0], dtype=torch.int8)
    matched_vals, matches = match_quality_matrix.max(dim=0)
    match_labels = torch.full((n,), 1, dtype=torch.int8)
    for l, low, high in zip(labels, th[:-1], th[1:]):
        match_labels[(matched_vals >= low) & (matched_vals < high)] = l
    if allow_low_quality_matches:
        highest_quality_foreach_gt, _ = match_quality_matrix.max(dim=1)
        _, pred_inds = torch.nonzero(match_quality_matrix == highest_quality_foreach_gt[:, None], as_tuple=True)
        match_labels[pred_inds] = 1
    return matches, match_labels


def default_perm(generator: Optional[torch.Generator] = None) -> Perm:
    return lambda n: torch.randperm(n, generator=generator)


def subsample_labels(labels: Tensor, num_samples: int, positive_fraction: float, bg_label: int, perm: Perm) -> Tuple[Tensor, Tensor]:
    """``subsample_labels``: indices of the sampled positives and negatives."""
    positive = torch.nonzero((labels != -1) & (labels != bg_label), as_tuple=True)[0]
    negative = torch.nonzero(labels == bg_label, as_tuple=True)[0]
    num_pos = min(positive.numel(), int(num_samples * positive_fraction))
    num_neg = min(negative.numel(), num_samples - num_pos)
    return positive[perm(positive.numel())[:num_pos]], negative[perm(negative.numel())[:num_neg]]


def get_deltas(src: Tensor, tgt: Tensor, weights: Sequence[float]) -> Tensor:
    """``Box2BoxTransform.get_deltas``."""
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = tgt[:, 2] - tgt[:, 0], tgt[:, 3] - tgt[:, 1]
    tcx, tcy = tgt[:, 0] + 0.5 * tw, tgt[:, 1] + 0.5 * th
    wx, wy, ww, wh = weights
    return torch.stack([wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)], dim=1)


def smooth_l1_sum(x: Tensor, t: Tensor, beta: float) -> Tensor:
    """fvcore ``smooth_l1_loss(reduction="sum")``: plain L1 below beta 1e-5."""
    d = (x - t).abs()
    if beta < 1e-5:
        return d.sum()
    return torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum()


# =====================================================================================
# RPN targets and losses  [EXT d2: modeling/proposal_generator/rpn.py]
# =====================================================================================
def rpn_label_and_sample_anchors(anchors: Tensor, gt_boxes: Sequence[Tensor], ts: TrainSpec, perm: Perm) -> Tuple[List[Tensor], List[Tensor]]:
    """``RPN.label_and_sample_anchors``: per image labels (A,) in {1, 0, -1} after subsampling and the matched gt
    box of every anchor (zeros when the image has no gt)."""
    labels, matched = [], []
    for gt in gt_boxes:
        idx, lab = matcher(pairwise_iou(gt, anchors), ts.rpn_iou_thresholds, ts.rpn_iou_labels, True)
        pos, neg = subsample_labels(lab, ts.rpn_batch_size_per_image, ts.rpn_positive_fraction, 0, perm)
        out = torch.full_like(lab, -1)
        out[pos] = 1
        out[neg] = 0
        labels.append(out)
        matched.append(gt[idx] if gt.shape[0] else torch.zeros_like(anchors))
    return labels, matched


def rpn_losses(anchors: Tensor, logits: Tensor, deltas: Tensor, labels: Sequence[Tensor], matched_gt: Sequence[Tensor], ts: TrainSpec) -> Dict[str, Tensor]:
    """``RPN.losses``.  logits (N, A_total), deltas (N, A_total, 4) in the (level, y, x, a) order of ``anchors``."""
    n = len(labels)
    gl = torch.stack(list(labels))
    pos, valid = gl == 1, gl >= 0
    tgt = torch.stack([get_deltas(anchors, m, ts.rpn_bbox_reg_weights) if bool((l == 1).any()) else torch.zeros_like(anchors)
                       for m, l in zip(matched_gt, labels)])
    loc = smooth_l1_sum(deltas[pos], tgt[pos], ts.rpn_smooth_l1_beta)
    cls = F.binary_cross_entropy_with_logits(logits[valid], gl[valid].to(torch.float32), reduction="sum")
    norm = ts.rpn_batch_size_per_image * n
    return {"loss_rpn_cls": cls / norm, "loss_rpn_loc": loc / norm}


# =====================================================================================
# ROI heads: proposal sampling and losses  [EXT d2: modeling/roi_heads/{roi_heads,fast_rcnn,mask_head}.py]
# =====================================================================================
def label_and_sample_proposals(proposals: Tensor, gt_boxes: Tensor, gt_classes: Tensor, num_classes: int, ts: TrainSpec,
                               perm: Perm) -> Dict[str, Tensor]:
    """``ROIHeads.label_and_sample_proposals`` for one image: gt boxes appended to the proposals (R:193), IoU matcher at
    0.5 without low-quality matches, ``roi_batch_size_per_image`` samples with at most 25 % foreground (foreground
    first).  Returns the sampled boxes, their classes (``num_classes`` = background) and matched gt index."""
    if ts.roi_proposal_append_gt:
        proposals = torch.cat([proposals, gt_boxes], 0)
    idx, lab = matcher(pairwise_iou(gt_boxes, proposals), [ts.roi_iou_threshold], [0, 1], False)
    if gt_classes.numel() > 0:
        cls = gt_classes[idx].clone()
        cls[lab == 0] = num_classes
        cls[lab == -1] = -1
    else:
        cls = torch.zeros_like(idx) + num_classes
    fg, bg = subsample_labels(cls, ts.roi_batch_size_per_image, ts.roi_positive_fraction, num_classes, perm)
    sel = torch.cat([fg, bg], 0)
    return {"boxes": proposals[sel], "classes": cls[sel], "gt_index": idx[sel], "sampled": sel}


def fast_rcnn_losses(scores: Tensor, deltas: Tensor, proposals: Tensor, gt_classes: Tensor, gt_boxes: Tensor, num_classes: int,
                     reg_weights: Sequence[float], ts: TrainSpec) -> Dict[str, Tensor]:
    """``FastRCNNOutputLayers.losses``: mean cross-entropy over all sampled RoIs; class-specific L1 on the foreground
    rows divided by the number of sampled RoIs."""
    loss_cls = F.cross_entropy(scores, gt_classes, reduction="mean")
    fg = torch.nonzero((gt_classes >= 0) & (gt_classes < num_classes), as_tuple=True)[0]
    pred = deltas.view(-1, num_classes, 4)[fg, gt_classes[fg]]
    loss_reg = smooth_l1_sum(pred, get_deltas(proposals[fg], gt_boxes[fg], reg_weights), ts.box_smooth_l1_beta)
    return {"loss_cls": loss_cls, "loss_box_reg": loss_reg / max(gt_classes.numel(), 1.0)}


def mask_rcnn_loss(mask_logits: Tensor, gt_classes: Tensor, gt_masks: Tensor) -> Tensor:
    """``mask_rcnn_loss``: BCE-with-logits (mean) of the gt class' logits (n,K,S,S) vs the rasterised gt masks (n,S,S)."""
    if mask_logits.shape[0] == 0:
        return mask_logits.sum() * 0
    sel = mask_logits[torch.arange(mask_logits.shape[0]), gt_classes]
    return F.binary_cross_entropy_with_logits(sel, gt_masks.to(torch.float32), reduction="mean")


# =====================================================================================
# Ground-truth masks: PolygonMasks.crop_and_resize -> pycocotools frPyObjects / merge / decode
# [EXT d2: structures/masks.py rasterize_polygons_within_box, polygons_to_bitmask; EXT coco: common/maskApi.c rleFrPoly]
# =====================================================================================
def rle_from_polygon(xy: np.ndarray, h: int, w: int) -> np.ndarray:
    """``rleFrPoly`` restated: polygon (k,2) float64 in pixel coordinates -> column-major binary mask (h, w) uint8.
    The boundary is traced on a 5x up-sampled integer grid, the crossing points of every column are collected and the
    run-length encoding follows from their sorted positions (column-major, as COCO RLE)."""
    k = xy.shape[0]
    scale = 5.0
    x = [int(scale * xy[j, 0] + 0.5) for j in range(k)]
    y = [int(scale * xy[j, 1] + 0.5) for j in range(k)]
    x.append(x[0])
    y.append(y[0])
    u: List[int] = []
    v: List[int] = []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        s = (ye - ys) / dx if dx >= dy and dx > 0 else ((xe - xs) / dy if dy > 0 else 0.0)
        if dx >= dy:
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(ys + s * t + 0.5))
        else:
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + 0.5))
    pts: List[int] = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + 0.5) / scale - 0.5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + 0.5) / scale - 0.5
            yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
            yd = math.ceil(yd)
            pts.append(int(xd) * h + int(yd))
    pts.append(h * w)
    pts.sort()
    # positions -> run lengths (alternating 0-run, 1-run, ...), zero-length interior runs merged as maskApi.c does
    a = [pts[0]] + [pts[i] - pts[i - 1] for i in range(1, len(pts))]
    b: List[int] = []
    j = 0
    b.append(a[j]); j += 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j]); j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]; j += 1
    flat = np.zeros(h * w, np.uint8)
    pos, val = 0, 0
    for run in b:
        if val:
            flat[pos:pos + run] = 1
        pos += run
        val ^= 1
    return flat.reshape(w, h).T.copy()           # RLE is column-major


def polygons_to_bitmask(polygons: Sequence[np.ndarray], h: int, w: int) -> np.ndarray:
    """``polygons_to_bitmask``: union (``mask_util.merge``) of the rasterised polygons; each polygon a flat
    [x0,y0,x1,y1,...] array."""
    if len(polygons) == 0:
        return np.zeros((h, w), bool)
    m = np.zeros((h, w), np.uint8)
    for p in polygons:
        m |= rle_from_polygon(np.asarray(p, np.float64).reshape(-1, 2), h, w)
    return m.astype(bool)


def rasterize_polygons_within_box(polygons: Sequence[np.ndarray], box: np.ndarray, mask_size: int) -> np.ndarray:
    """``rasterize_polygons_within_box``: shift by the box origin, scale to mask_size (separate x/y ratios), rasterise."""
    w, h = box[2] - box[0], box[3] - box[1]
    polys = [np.asarray(p, np.float64).copy() for p in polygons]
    for p in polys:
        p[0::2] = p[0::2] - box[0]
        p[1::2] = p[1::2] - box[1]
    ratio_h = mask_size / max(h, 0.1)
    ratio_w = mask_size / max(w, 0.1)
    if ratio_h == ratio_w:
        for p in polys:
            p *= ratio_h
    else:
        for p in polys:
            p[0::2] *= ratio_w
            p[1::2] *= ratio_h
    return polygons_to_bitmask(polys, mask_size, mask_size)


# =====================================================================================
# Differentiable RoIAlign (same arithmetic as maskrcnn_oracle.roi_align_one, written with torch ops)
# =====================================================================================
def _axis_weights(start: float, bin_size: float, grid: int, P: int, size: int) -> np.ndarray:
    """(P, size) matrix: summed bilinear weights of the `grid` samples of every bin on every feature row/column,
    with torchvision's skip (outside [-1, size]) and clamp rules."""
    Wm = np.zeros((P, size), np.float32)
    f32 = np.float32
    for b in range(P):
        for i in range(grid):
            c = f32(start) + f32(b) * f32(bin_size) + (f32(i) + f32(0.5)) * f32(bin_size) / f32(grid)
            if c < -1.0 or c > size:
                continue
            c = max(c, f32(0.0))
            lo = int(c)
            if lo >= size - 1:
                hi = lo = size - 1
                c = f32(lo)
            else:
                hi = lo + 1
            l = f32(c) - f32(lo)
            Wm[b, lo] += f32(1.0) - l
            Wm[b, hi] += l
    return Wm


def roi_align_diff(feat: Tensor, roi: Tensor, out_size: int, spatial_scale: float) -> Tensor:
    """RoIAlign(aligned=True, sampling_ratio=0) of one RoI on feat (C,H,W), differentiable w.r.t. ``feat``: the bin
    average over its samples is separable, out = Wy @ feat @ Wx^T / count."""
    C, H, W = feat.shape
    f32 = np.float32
    sc = f32(spatial_scale)
    r = roi.detach().numpy().astype(np.float32)
    sw, sh = r[0] * sc - f32(0.5), r[1] * sc - f32(0.5)
    rw, rh = (r[2] * sc - f32(0.5)) - sw, (r[3] * sc - f32(0.5)) - sh
    bh, bw = rh / f32(out_size), rw / f32(out_size)
    gh, gw = max(int(math.ceil(rh / f32(out_size))), 0), max(int(math.ceil(rw / f32(out_size))), 0)
    count = max(gh * gw, 1)
    Wy = torch.from_numpy(_axis_weights(sh, bh, gh, out_size, H)).to(feat.dtype)      # fp32 weights; float64 maps take them exactly
    Wx = torch.from_numpy(_axis_weights(sw, bw, gw, out_size, W)).to(feat.dtype)
    return torch.einsum("ph,chw,qw->cpq", Wy, feat, Wx) / count


def roi_pooler_diff(feats: Sequence[Tensor], scales: Sequence[float], boxes: Tensor, image_index: Tensor, out_size: int) -> Tensor:
    lv = O.assign_levels(boxes, 2, 5)
    outs = [roi_align_diff(feats[int(lv[r])][int(image_index[r])], boxes[r], out_size, scales[int(lv[r])]) for r in range(boxes.shape[0])]
    if not outs:
        return torch.zeros((0, feats[0].shape[1], out_size, out_size))
    return torch.stack(outs)


# =====================================================================================
# GeneralizedRCNN.forward (training)  [EXT d2: modeling/meta_arch/rcnn.py]
# =====================================================================================
def trainable_keys(W: Dict[str, Tensor], freeze_at: int = 2) -> List[str]:
    """Parameters that receive gradients: everything except FrozenBN statistics/affine (no parameters at all in d2) and
    the stem + res2 when FREEZE_AT == 2 (R:58)."""
    out = []
    for k in W:
        if ".norm." in k:
            continue
        if k.startswith("backbone.bottom_up.stem.") and freeze_at >= 1:
            continue
        if k.startswith("backbone.bottom_up.res2.") and freeze_at >= 2:
            continue
        out.append(k)
    return out


def train_forward(spec: EngineSpec, ts: TrainSpec, W: Dict[str, Tensor], images: Tensor, image_sizes: Sequence[Tuple[int, int]],
                  gt_boxes: Sequence[Tensor], gt_classes: Sequence[Tensor], gt_polygons: Sequence[Sequence[Sequence[np.ndarray]]],
                  perm: Perm, proposals: Optional[Sequence[Tensor]] = None) -> Dict[str, Tensor]:
    """Losses of one training batch.  ``images``: normalised, padded (N,3,H,W) network input; gt boxes in network-input
    pixels.  ``proposals``: optional externally supplied RPN proposals per image (the parity tests hand the engine's own,
    since top-k / NMS are tested separately and are not differentiated through -- detectron2 detaches them too)."""
    feats = O.resnet_forward(spec, W, images)
    feats.update(O.fpn_forward(spec, W, feats))
    rpn_feats = [feats[n] for n in spec.rpn_in_features]
    logits, deltas = O.rpn_head(W, rpn_feats)
    anchors = torch.cat([O.grid_anchors(spec, l, f.shape[2], f.shape[3]) for l, f in enumerate(rpn_feats)])
    N = images.shape[0]
    lg = torch.cat([x.permute(0, 2, 3, 1).reshape(N, -1) for x in logits], 1)
    dl = torch.cat([x.view(N, -1, 4, x.shape[2], x.shape[3]).permute(0, 3, 4, 1, 2).reshape(N, -1, 4) for x in deltas], 1)
    labels, matched = rpn_label_and_sample_anchors(anchors, gt_boxes, ts, perm)
    losses = rpn_losses(anchors, lg, dl, labels, matched, ts)
    if proposals is None:
        with torch.no_grad():
            train_spec = spec.replace(rpn_pre_nms_topk_test=ts.rpn_pre_nms_topk_train, rpn_post_nms_topk_test=ts.rpn_post_nms_topk_train)
            props = O.rpn_proposals(train_spec, [l.detach() for l in logits], [d.detach() for d in deltas], image_sizes, nms_trick=False)
            proposals = [p["boxes"] for p in props]
    K = spec.num_classes
    samples = [label_and_sample_proposals(proposals[n], gt_boxes[n], gt_classes[n], K, ts, perm) for n in range(N)]
    roi_feats = [feats[n] for n in spec.roi_in_features]
    scales = [1.0 / s for s in spec.fpn_strides[: len(roi_feats)]]
    boxes = torch.cat([s["boxes"] for s in samples])
    img_idx = torch.cat([torch.full((s["boxes"].shape[0],), n, dtype=torch.int64) for n, s in enumerate(samples)])
    cls = torch.cat([s["classes"] for s in samples])
    gtb = torch.cat([gt_boxes[n][s["gt_index"]] if gt_boxes[n].shape[0] else s["boxes"] for n, s in enumerate(samples)])
    pooled = roi_pooler_diff(roi_feats, scales, boxes, img_idx, spec.box_pooler_resolution)
    _, sc, reg = O.box_head(W, pooled)
    losses.update(fast_rcnn_losses(sc, reg, boxes, cls, gtb, K, spec.box_reg_weights, ts))
    if spec.mask_on:
        fg = torch.nonzero((cls >= 0) & (cls < K), as_tuple=True)[0]
        mp = roi_pooler_diff(roi_feats, scales, boxes[fg], img_idx[fg], spec.mask_pooler_resolution)
        mlog, _ = O.mask_head(spec, W, mp, cls[fg])
        S = mlog.shape[-1] if mlog.shape[0] else 2 * spec.mask_pooler_resolution
        gidx = torch.cat([s["gt_index"] for s in samples])[fg]
        gm = [rasterize_polygons_within_box(gt_polygons[int(img_idx[r])][int(gi)], boxes[r].numpy(), S) for r, gi in zip(fg.tolist(), gidx.tolist())]
        gmt = torch.from_numpy(np.stack(gm)) if gm else torch.zeros((0, S, S), dtype=torch.bool)
        losses["loss_mask"] = mask_rcnn_loss(mlog, cls[fg], gmt)
    losses["_samples"] = samples            # for the parity tests (same sampled sets on both sides)
    losses["_rpn_labels"] = labels
    return losses


# =====================================================================================
# Solver  [EXT d2: solver/{build,lr_scheduler}.py]
# =====================================================================================
def lr_at(ts: TrainSpec, it: int) -> float:
    """``WarmupMultiStepLR``: base_lr * warmup(it) * gamma ** (number of milestones <= it); linear warm-up from
    ``warmup_factor`` over ``warmup_iters`` iterations."""
    if it < ts.warmup_iters:
        alpha = it / ts.warmup_iters
        wf = ts.warmup_factor * (1 - alpha) + alpha
    else:
        wf = 1.0
    return ts.base_lr * wf * ts.gamma ** sum(1 for s in ts.steps if s <= it)
