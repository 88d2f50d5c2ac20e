"""detectron2 0.6's training diagnostics as integer counts, in numpy: the reference of tests/test_train_stats_cpu.py and
tests/test_gpu_train_stats.py.  ``np.argmax`` is the first maximum (torch.argmax), the comparisons run on float32 arrays.

    RPN.losses                                   pos = #(label == 1), neg = #(label == 0)
    label_and_sample_proposals                   fg / bg = sums of the sampled counts per image
    FastRCNNOutputLayers._log_classification_stats
                                                 rows with 0 <= class <= K: inst, correct (pred == class), fgn (class < K),
                                                 fg_correct, fg_as_bg (foreground rows predicted K)
    mask_rcnn_loss                               pixels of the first min(total, capacity) entries whose class is in [0, cs):
                                                 p = logit[class] > 0, g = target != 0 -> pixels, p != g, g, p & ~g, ~p & g
"""
import numpy as np


def label_counts(labels):
    l = np.asarray(labels, np.int32).reshape(-1)
    return np.array([(l == 1).sum(), (l == 0).sum()], np.int32)


def box_stats(pred, gt_classes, K, sampled_counts=None):
    """pred (n_rois, cs) float32, gt_classes (n_rois,) -> int32 [7]: fg, bg, inst, correct, fgn, fg_correct, fg_as_bg."""
    pred = np.asarray(pred, np.float32).reshape(len(gt_classes), -1)
    cls = np.asarray(gt_classes, np.int32)
    out = np.zeros(7, np.int32)
    if sampled_counts is not None:
        sc = np.asarray(sampled_counts, np.int32).reshape(-1, 2)
        out[0], out[1] = sc[:, 0].sum(), sc[:, 1].sum()
    valid = (cls >= 0) & (cls <= K)
    if valid.any():
        p = np.argmax(pred[valid][:, :K + 1], axis=1)
        c = cls[valid]
        fg = c < K
        out[2:] = [valid.sum(), (p == c).sum(), fg.sum(), (fg & (p == c)).sum(), (fg & (p == K)).sum()]
    return out


def mask_stats(logits, targets, gt_classes, total=None):
    """logits (n_masks, side*side, cs) float32, targets (n_masks, side*side) uint8, gt_classes (n_masks,) -> int32 [5]."""
    logits = np.asarray(logits, np.float32)
    cap, _, cs = logits.shape
    n = cap if total is None else min(int(total), cap)
    out = np.zeros(5, np.int64)
    for m in range(max(n, 0)):
        c = int(gt_classes[m])
        if not 0 <= c < cs:
            continue
        p = logits[m, :, c] > np.float32(0.0)
        g = np.asarray(targets[m]).reshape(-1) != 0
        out += [p.size, (p != g).sum(), g.sum(), (p & ~g).sum(), (~p & g).sum()]
    return out.astype(np.int32)


def table(rpn_labels, roi_classes, sampled_count, box_pred, K, mask_logits=None, mask_targets=None, mask_classes=None, mask_total=0):
    """The trainer's int32 [16] table of a step over its n images (every array already cut to them)."""
    n = len(rpn_labels)
    t = np.zeros(16, np.int32)
    t[0:2] = label_counts(rpn_labels)
    t[2:9] = box_stats(np.asarray(box_pred).reshape(-1, np.asarray(box_pred).shape[-1]), np.asarray(roi_classes).reshape(-1), K, sampled_count)
    if mask_logits is not None:
        t[9:14] = mask_stats(mask_logits, mask_targets, mask_classes, mask_total)
    t[14] = n
    return t
