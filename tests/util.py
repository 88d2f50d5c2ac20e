"""Shared helpers for the parity tests (synthetic tiles, detection matching)."""
import numpy as np


from proj_roadsurf_amd.synthetic import synthetic_scenes, synthetic_tiles  # noqa: F401  (one definition, in the package)


from proj_roadsurf_amd.matching import box_iou, match_detections, wilson_lower  # noqa: F401  (one definition, in the package)


def conv_stage_shapes(spec, net_h=800, net_w=800):
    """(stage name, output pixels per tile, cin, k, cout, cin2, forced variant or None) of every GEMM stage of the fp16
    inference engine, in execution order -- the host-side mirror of csrc/engine.hip's builder sections (declared in csrc/engine_internal.h: rs_engine::build_stem,
    build_bottleneck / add_fused_tail, build_fpn, build_rpn, build_box_head, build_mask_head) that the tile-dispatch tests enumerate.  Output pixels per tile times the batch size is the GEMM's M."""
    out = []
    h2, w2, h4, w4 = net_h // 2, net_w // 2, net_h // 4, net_w // 4
    out.append(("stem.conv1+maxpool", h2 * w2, 4, 7, spec.stem_out_channels, 0, 21))     # csrc/stem_fused.hip
    cur_c, bott, cout, ch, cw = spec.stem_out_channels, 64, spec.res2_out_channels, h4, w4
    have_t1 = False
    for si, nb in enumerate(spec.res_blocks):
        for bi in range(nb):
            nm = f"res{si + 2}.{bi}"
            stride = 2 if (bi == 0 and si > 0) else 1
            s1 = stride if spec.stride_in_1x1 else 1
            oh, ow = ch // stride, cw // stride
            proj = cur_c != cout
            tail = stride == 1 and ((bott == 64 and cout == 256) or (bott == 128 and cout == 512 and bi > 0))    # fused tails (csrc/bneck_fused.hip), variant 13
            if not have_t1:
                out.append((nm + ".conv1", (ch // s1) * (cw // s1), cur_c, 1, bott, 0, None))
            have_t1 = False
            if tail:
                have_t1 = bi + 1 < nb
                out.append((nm + (".conv2+conv3+next.conv1" if have_t1 else ".conv2+conv3"), oh * ow, bott, 3, cout, 0, 13))
            else:
                out.append((nm + ".conv2", oh * ow, bott, 3, bott, 0, None))
                out.append((nm + ".conv3", oh * ow, bott, 1, cout, cur_c if proj else 0, None))
            cur_c, ch, cw = cout, oh, ow
        bott *= 2
        cout *= 2
    sizes = [(h4 >> l, w4 >> l) for l in range(4)]
    res_c = [spec.res2_out_channels * (2 ** i) for i in range(4)]
    for l in (3, 2, 1, 0):
        out.append((f"fpn_lateral{l + 2}", sizes[l][0] * sizes[l][1], res_c[l], 1, 256, 0, None))
    # the 3x3 output convolutions of the four levels, and the shared RPN 3x3 over the five, run as ONE multi-map conv_deep launch
    # each (launch_conv_deep_multi; variant 12 at every batch size)
    out.append(("fpn_output2-5", sum(a * b for a, b in sizes), 256, 3, 256, 0, 12))
    p6 = ((sizes[3][0] - 1) // 2 + 1, (sizes[3][1] - 1) // 2 + 1)
    # ... with the 16-row objectness + delta head inside its epilogue (ConvParams::head_w): no rpn.heads stages
    out.append(("rpn.conv+heads2-6", sum(a * b for a, b in sizes + [p6]), 256, 3, 256, 0, 12))
    pr, fc = spec.box_pooler_resolution, spec.box_fc_dim
    out.append(("box.fc1", 1024, pr * pr * 256, 1, fc, 0, None))
    out.append(("box.fc2", 1024, fc, 1, fc, 0, None))
    out.append(("box.predictor", 1024, fc, 1, 16, 0, 2))
    if spec.mask_on:
        mr, d = spec.mask_pooler_resolution, spec.detections_per_image
        for i in range(spec.mask_num_conv):
            out.append((f"mask.fcn{i + 1}", d * mr * mr, 256, 3, 256, 0, None))
        out.append(("mask.deconv_predict", d * mr * mr, 256, 1, 256, 0, 22))     # csrc/conv_wreg.hip, EPI 3
    return out


# ------------------------------------------------------------------ detection edges: FPN level cut points, NMS threshold
_F32 = np.float32
FPN_CUTS = (0.5, 1.0, 2.0)        # v at the level boundaries of floor(4 + log2(v)) in exact arithmetic


def f32_steps(x, lo, hi):
    """The float32 values from `lo` floats below x to `hi` floats above it (x itself rounded to float32), ascending."""
    x = _F32(x)
    below, above = [], []
    a = b = x
    for _ in range(lo):
        a = np.nextafter(a, _F32(-np.inf))
        below.append(a)
    for _ in range(hi):
        b = np.nextafter(b, _F32(np.inf))
        above.append(b)
    return np.array(below[::-1] + [x] + above, np.float32)


def fpn_level_v(boxes):
    """v = sqrt(area) / 224 + 1e-8 in fp32, in detectron2's operation order (assign_boxes_to_levels)."""
    b = np.asarray(boxes, np.float32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore"):
        return (np.sqrt(area) / _F32(224)).astype(np.float32) + _F32(1e-8)


def fpn_level_ref(boxes):
    """detectron2's floor(4 + log2(v)) clamped to [2, 5], minus 2, in fp32 with a correctly rounded log2: the float64 log2
    rounded to fp32, then the fp32 add and the floor."""
    v = fpn_level_v(boxes)
    with np.errstate(divide="ignore"):
        lg = np.log2(v.astype(np.float64)).astype(np.float32)
    return np.clip(np.floor(_F32(4) + lg), 2, 5).astype(np.int64) - 2


def fpn_level_pow2_rule(boxes):
    """The rule the kernels used before: v >= 0.5 / 1 / 2 (kept to show that the sweep reaches where it differs)."""
    v = fpn_level_v(boxes)
    return np.where(v >= 2, 3, np.where(v >= 1, 2, np.where(v >= 0.5, 1, 0))).astype(np.int64)


def fpn_level_window(cut, k=16):
    """The 2k+1 float32 values of v from k floats below `cut` to k above, and the subset that a box can produce at all:
    v = fl(fl(s / 224) + 1e-8) for a float32 sqrt(area) s (below each cut the v grid is finer than the grid of s / 224,
    so one or two of the floats are unreachable by any box)."""
    win = f32_steps(cut, k, k)
    s = f32_steps(224.0 * cut, 4 * k + 8, 4 * k + 8)
    reach = set((s / _F32(224)).astype(np.float32) + _F32(1e-8))
    return win, np.array([w for w in win if w in reach], np.float32)


def fpn_level_sweep_boxes(k_steps=96):
    """Boxes whose v steps one float at a time across each cut v in {0.5, 1, 2}: one edge of a box of side 224 * cut is moved
    one float32 at a time, with x1 = y1 = 0 and with non-integer x1 / y1 (the subtraction rounds as well), plus squares whose
    two far edges move together."""
    out = []
    for cut in FPN_CUTS:
        s0 = 224.0 * cut
        for x1, y1 in ((0.0, 0.0), (0.37, 1.61), (13.3, 7.9)):
            x2s = f32_steps(x1 + s0, k_steps, k_steps)
            y2 = _F32(y1 + s0)
            out += [[x1, y1, x2, y2] for x2 in x2s]
        for e in f32_steps(s0, k_steps, k_steps):
            out.append([0.0, 0.0, e, e])
    return np.array(out, np.float32)


def fpn_level_edge_boxes(seed=0, n_random=512):
    """The sweep, degenerate boxes (area 0), very large boxes (clamped to p5) and random boxes over all scales."""
    rng = np.random.default_rng(seed)
    sweep = fpn_level_sweep_boxes()
    degenerate = np.array([[5, 5, 5, 9], [3, 3, 3, 3], [0, 0, 100, 0], [17.5, 40.25, 17.5, 40.25]], np.float32)
    large = np.array([[0, 0, 1800, 1800], [-100, -80, 1500, 1200], [0, 0, 2000, 700], [10, 10, 900, 1900]], np.float32)
    side = np.exp(rng.uniform(np.log(1.0), np.log(1400.0), (n_random, 2)))
    xy = rng.uniform(-50, 500, (n_random, 2))
    rand = np.concatenate([xy, xy + side], 1).astype(np.float32)
    return np.concatenate([sweep, degenerate, large, rand]).astype(np.float32)


def nms_iou32(a, b):
    """fp32 IoU of boxes a, b (rows) in torchvision's operation order (devIoU / nms_kernel.cpp)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    w = np.maximum(_F32(0), np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    h = np.maximum(_F32(0), np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    inter = w * h
    sa = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    sb = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / (sa + sb - inter)).astype(np.float32), inter.astype(np.float32), (sa + sb - inter).astype(np.float32)


def nms_iou_class(a, b, t):
    """Where each pair (a, b) lies relative to threshold t: 'eq' / 'up' / 'down' (fp32 IoU == float32(t) / the next float
    above / below), 'band' (inside the kernel's +-1e-5 relative division band around thr * union, off those three),
    'out_hi' / 'out_lo' (within 3e-5 of t but outside the band), else 'far'.  thr is the value the host passes."""
    from proj_roadsurf_amd.engine import nms_thresh_f32
    iou, inter, uni = nms_iou32(a, b)
    ft = _F32(t)
    tu = _F32(nms_thresh_f32(t)) * uni
    with np.errstate(invalid="ignore"):
        rel = iou.astype(np.float64) / t - 1
    cls = np.where(iou == ft, "eq", np.where(iou == np.nextafter(ft, _F32(np.inf)), "up",
                   np.where(iou == np.nextafter(ft, _F32(-np.inf)), "down",
                   np.where((inter > tu * _F32(0.99999)) & ~(inter > tu * _F32(1.00001)), "band",
                   np.where(np.abs(rel) < 3e-5, np.where(rel > 0, "out_hi", "out_lo"), "far")))))
    return cls


NMS_EDGE_CLASSES = ("eq", "up", "down", "band", "out_hi", "out_lo")


def nms_edge_pairs(t, cell=100.0, grid=8):
    """Pairs (A, B) in disjoint cells of a grid x grid field of `cell`-px cells (coordinates up to grid * cell = 800 px): B
    shares A's x1 and y1; its x2 and y2 are searched one float32 at a time so that the fp32 IoU lands on each class of
    nms_iou_class for threshold t, for an integer and a non-integer A; plus an identical pair and a zero-area pair.
    Returns (boxes [2 * pairs][4] in priority order A0, B0, A1, B1, ...), classes [pairs])."""
    pairs, classes = [], []
    cells = iter([(cx * cell, cy * cell) for cy in range(grid) for cx in range(grid)][::-1])   # the 800-px corner first
    targets = {"eq": 1.0, "up": 1.0, "down": 1.0, "band": 1 - 6e-6, "out_hi": 1 + 1.6e-5, "out_lo": 1 - 1.6e-5}
    shapes = {"int": [(90.0, 80.0, 3.0, 5.0), (64.0, 48.0, 1.0, 2.0), (96.0, 77.0, 0.0, 4.0), (50.0, 75.0, 10.0, 10.0), (33.0, 95.0, 7.0, 1.0)],
              "frac": [(87.37, 91.61, 2.25, 4.8125), (61.5, 73.25, 1.5, 3.75), (44.1, 59.9, 0.3, 8.7), (93.3, 38.45, 5.55, 2.2)]}
    for kind, geoms in shapes.items():
        for want, rel in targets.items():
            cx, cy = next(cells)
            for w, h, ox, oy in geoms:
                A = np.array([cx + ox, cy + oy, cx + ox + w, cy + oy + h], np.float32)
                y2s = f32_steps(float(A[1]) + h * t * rel, 300, 300)
                x2s = f32_steps(float(A[2]), 128, 0)
                Y, X = np.meshgrid(y2s, x2s, indexing="ij")
                B = np.stack([np.full(Y.shape, A[0]), np.full(Y.shape, A[1]), X, Y], -1).reshape(-1, 4).astype(np.float32)
                hit = np.nonzero(nms_iou_class(A[None], B, t) == want)[0]
                if len(hit):
                    pairs.append((A, B[hit[len(hit) // 2]]))
                    classes.append(want)
                    break
    cx, cy = next(cells)
    A = np.array([cx + 10.5, cy + 20, cx + 70, cy + 95.25], np.float32)
    pairs.append((A, A.copy()))
    classes.append("identical")
    cx, cy = next(cells)
    z = np.array([cx + 5, cy + 5, cx + 5, cy + 60], np.float32)
    pairs.append((z, z.copy()))
    classes.append("zero_area")
    boxes = np.stack([b for p in pairs for b in p]).astype(np.float32)
    return boxes, classes


def fpn_level_boundary_boxes(per_cut=2):
    """Boxes of the sweep on which detectron2's level and the old `v >= 2^k` rule differ: `per_cut` of them at each cut."""
    b = fpn_level_sweep_boxes()
    v = fpn_level_v(b)
    differ = fpn_level_ref(b) != fpn_level_pow2_rule(b)
    out = []
    for cut in FPN_CUTS:
        idx = np.nonzero(differ & (np.abs(v - cut) < 1e-5))[0]
        out += [b[i] for i in idx[:: max(1, len(idx) // per_cut)][:per_cut]]
    return np.array(out, np.float32)


def roi_grid(box, P, sc, H, W):
    """(gh, gw) of torchvision's adaptive sampling and the feature-cell window [y0, y1) x [x0, x1) the RoI's samples can touch."""
    f32 = np.float32
    x1, y1, x2, y2 = (f32(v) for v in box)
    sw, sh = f32(x1 * f32(sc) - f32(0.5)), f32(y1 * f32(sc) - f32(0.5))
    ew, eh = f32(x2 * f32(sc) - f32(0.5)), f32(y2 * f32(sc) - f32(0.5))
    gh = max(int(np.ceil(float(f32(f32(eh - sh) / f32(P))))), 0)
    gw = max(int(np.ceil(float(f32(f32(ew - sw) / f32(P))))), 0)
    y0, x0 = int(np.clip(np.floor(sh), 0, H - 1)), int(np.clip(np.floor(sw), 0, W - 1))
    yb, xb = int(np.clip(np.floor(eh) + 2, 1, H)), int(np.clip(np.floor(ew) + 2, 1, W))
    return gh, gw, (y0, max(yb, y0 + 1)), (x0, max(xb, x0 + 1))
