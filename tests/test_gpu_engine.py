"""GPU parity of the whole engine, through the C ABI, against the CPU oracle.

Two kinds of checks:

* stage-wise: every stage of the forward is re-computed by the oracle FROM THE ENGINE'S OWN
  INPUT to that stage (read back through ``rs_engine_tensor``), so discrete stages (top-k, NMS,
  level assignment, thresholds) must agree exactly and float stages within the tolerance written
  next to each assert;
* end-to-end: oracle fp32 forward vs engine (fp16 operands / fp32 accumulate) on the same tiles and weights, detections
  matched greedily by class + IoU >= 0.95.  SURVEY.md §8d's tolerance is >= 98 % matched both ways, |dscore| <= 0.02,
  mask IoU >= 0.95.  Two workloads:
  - TRAINED-LIKE weights (proj_roadsurf_amd.synthetic.train_trained_like: the repo's own trainer, 600 SGD steps on
    synthetic scenes): the fp16 engine MEETS the tolerance -- asserted on a pool of four training seeds x 48 scenes (>= 1500
    detections) together with the Wilson lower bound of the matched fraction
    (`test_fp16_meets_the_stated_tolerance_on_a_trained_like_detector`; measured values in profiles/r03/parity/).
  - RANDOM weights (weights.synthetic_weights): every proposal regresses to a box of its own and the top-100 scores lie
    within a few percent of each other, so the detection set is chaotic in the features: re-running the ORACLE ITSELF on its
    own fp32 FPN maps plus relative Gaussian noise loses 2-6 % of the detections at 3e-4 noise and is back at 98-100 % only
    at 1e-4 (tools/parity/noise_sensitivity.py, profiles/r02/parity/noise_random.json), and the oracle downstream of the
    engine's fp16 FPN maps (rel. error 1e-3, everything after the backbone in fp32) already differs in 3-14 %
    (tools/parity/bisect.py, profiles/r02/parity/bisect_random.json).  The detections that differ already differ there: the
    loss is in the fp16 storage of the trunk (the same finding, stage by stage, on the trained-like workload: tools/parity/
    bisect_stages.py, profiles/r03/parity/).  Measured: 85-95 % matched,
    |dscore| <= 1e-3.  These tests assert >= 0.85 on the fp16 engine and the strict bar on the reference-precision (fp32
    MFMA) mode, which is what pins the engine's LOGIC on this workload (100 % matched, |dscore| <= 2e-6).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd.engine import Engine
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests.util import match_detections, roi_grid as _roi_grid, synthetic_tiles

pytestmark = pytest.mark.gpu


def _oracle():
    from oracle import maskrcnn_oracle as O
    return O


def _r16w(W):
    """weights as the engine sees them (fp16-rounded), for stage tests of GEMM stages"""
    return {k: torch.from_numpy(np.asarray(v)).half().float() for k, v in W.items()}


@pytest.fixture(scope="module")
def small(gpu_required):
    """256x256 tiles resized to 320x320 (p2 80x80 ... p6 3x3), 300 proposals, batch 3."""
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    eng = Engine(spec, W, (256, 256, 3), max_batch=4)
    dets = eng.infer(tiles, want_probs=True)
    yield spec, W, tiles, eng, dets
    eng.close()


def test_preprocess_bit_exact(small):
    spec, W, tiles, eng, _ = small
    O = _oracle()
    x = eng.tensor("net_input", n=3)           # (3, 320, 320, 4) fp16
    for i in range(3):
        t, _ = O.predictor_preprocess(spec, tiles[i])
        ref, _ = O.normalize_and_pad(spec, [t])
        ref16 = ref[0].permute(1, 2, 0).half().numpy()
        assert np.array_equal(x[i, :, :, :3], ref16), "resize + normalisation must be bit-exact with PIL + fp32 math"
        assert not x[i, :, :, 3:].any()


def test_backbone_features(small):
    spec, W, tiles, eng, _ = small
    O = _oracle()
    m = O.OracleModel(spec, W)
    x = torch.from_numpy(eng.tensor("net_input", n=3)[..., :3].astype(np.float32)).permute(0, 3, 1, 2)
    feats = m.backbone(x)
    # fp16 storage of every activation + fp16 weights: relative L2 error per map <= 1.5 %
    for name in ["stem", "res2", "res3", "res4", "res5", "p2", "p3", "p4", "p5", "p6"]:
        got = torch.from_numpy(eng.tensor(name, n=3).astype(np.float32)).permute(0, 3, 1, 2)
        ref = feats[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        rel = float((got - ref).norm() / ref.norm())
        assert rel <= 1.5e-2, f"{name}: rel L2 err {rel}"


# ---------------------------------------------------------------- stage checks on an engine after a forward of n tiles
FEAT_SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]


def _rpn_inputs(spec, eng, n):
    A = spec.num_anchors
    logits, deltas = [], []
    for l in range(len(spec.rpn_in_features)):
        h = torch.from_numpy(eng.tensor(f"rpn_head{l + 2}", n=n))          # (n,H,W,16) fp32
        logits.append(h[..., :A].permute(0, 3, 1, 2).contiguous())
        deltas.append(h[..., A:5 * A].permute(0, 3, 1, 2).contiguous())
    return logits, deltas


def check_rpn_stage(spec, eng, n):
    """RPN top-k sets and order per (image, level), proposal count, logits (exact) and boxes (1e-3 px), against the oracle on the
    engine's own head outputs.  Returns the oracle's per-image result."""
    O = _oracle()
    logits, deltas = _rpn_inputs(spec, eng, n)
    nh, nw, _, _ = eng.net_shape()
    ref = O.rpn_proposals(spec, logits, deltas, [(nh, nw)] * n, nms_trick=False)
    pb = eng.tensor("proposal_boxes", n=n)
    pl = eng.tensor("proposal_logits", n=n)
    pc = eng.tensor("proposal_count", n=n)
    cidx = eng.tensor("rpn_cand_index", n=n)
    ccount = eng.tensor("rpn_cand_count", n=n)
    for i in range(n):
        # top-k selection (index work): exact
        off = 0
        for l in range(len(logits)):
            k = int(ccount[i, l])
            want = ref[i]["pre_nms"]["anchor_idx"][off:off + k].numpy()
            assert np.array_equal(cidx[i, l, :k], want), f"image {i} level {l}: top-k anchor set/order differs"
            off += k
        m = int(pc[i])
        assert m == ref[i]["boxes"].shape[0], f"image {i}: {m} proposals vs {ref[i]['boxes'].shape[0]}"
        # logits are copied, not computed: exact.  Boxes go through expf: 1e-3 px.
        assert np.array_equal(pl[i, :m], ref[i]["logits"].numpy())
        assert np.abs(pb[i, :m] - ref[i]["boxes"].numpy()).max() <= 1e-3
    return ref


def rpn_topk_ties(spec, eng, n):
    """Per (image, level): (logits equal to the k-th largest, of them taken) where the level has more anchors than k."""
    logits, _ = _rpn_inputs(spec, eng, n)
    ccount = eng.tensor("rpn_cand_count", n=n)
    cidx = eng.tensor("rpn_cand_index", n=n)
    out = {}
    for i in range(n):
        for l, lg in enumerate(logits):
            v = lg[i].permute(1, 2, 0).flatten().numpy()
            k = int(ccount[i, l])
            if k == 0 or k >= v.size:
                continue
            kth = v[cidx[i, l, k - 1]]
            out[(i, l)] = (int((v == kth).sum()), int((v[cidx[i, l, :k]] == kth).sum()))
    return out


def nms_form(segments):
    """The NMS kernel's form for a launch of `segments` segments at cap 1024 (launch_nms; the engine always passes scratch)."""
    return "global" if segments <= 32 else "lds"


def check_rpn_nms(spec, eng, n):
    """rpn_cand_keep == the oracle's NMS over rpn_cand_boxes / rpn_cand_valid of each (image, level): exact."""
    O = _oracle()
    cb, cv = eng.tensor("rpn_cand_boxes", n=n), eng.tensor("rpn_cand_valid", n=n)
    ck, cc = eng.tensor("rpn_cand_keep", n=n), eng.tensor("rpn_cand_count", n=n)
    for i in range(n):
        for l in range(cc.shape[1]):
            c = int(cc[i, l])
            v = cv[i, l, :c].astype(bool)
            want = np.zeros(c, bool)
            want[np.nonzero(v)[0][O.nms_sorted_np(cb[i, l, :c][v], spec.rpn_nms_thresh)]] = True
            assert np.array_equal(ck[i, l, :c].astype(bool), want), f"image {i} level {l}: RPN NMS keep flags differ"
    return nms_form(n * cc.shape[1])


def check_box_nms(spec, eng, n):
    """box_seg_keep == the oracle's NMS over box_seg_boxes of each (image, class): exact."""
    O = _oracle()
    sb, sk, sc = eng.tensor("box_seg_boxes", n=n), eng.tensor("box_seg_keep", n=n), eng.tensor("box_seg_count", n=n)
    for i in range(n):
        for k in range(sc.shape[1]):
            c = int(sc[i, k])
            want = O.nms_sorted_np(sb[i, k, :c], spec.nms_thresh_test)
            assert np.array_equal(sk[i, k, :c].astype(bool), want), f"image {i} class {k}: box NMS keep flags differ"
    return nms_form(n * sc.shape[1])


def check_levels(eng, n):
    """box_roi_level == oracle.assign_levels of the proposals: exact."""
    O = _oracle()
    pb, pc, lv = eng.tensor("proposal_boxes", n=n), eng.tensor("proposal_count", n=n), eng.tensor("box_roi_level", n=n)
    for i in range(n):
        m = int(pc[i])
        assert np.array_equal(lv[i, :m], O.assign_levels(torch.from_numpy(pb[i, :m]), 2, 5).numpy()), f"image {i}: FPN level assignment must be exact"


def _check_pooled(O, feats_i, box, lvl, P, got, precision, ratios):
    """One RoI: fp16 -- the existing bound, 2e-3 * max(1, max|ref|) on the fp32 oracle; split / fp32 -- the oracle in float64 on
    the engine's own maps and the bound of the kernels' operation order:
    ((gh+2)(gw+2) + gh + gw + 4) * 2^-24 * max|F in the window| + s * |ref|, s = 2^-22 (two fp16 planes) or 2^-24 (fp32)."""
    F_ = feats_i[lvl]
    H, W = F_.shape[1:]
    if precision == "fp16":
        ref = O.roi_align_one(torch.from_numpy(F_), torch.from_numpy(box), P, FEAT_SCALES[lvl])
        assert float((got - ref).abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max()))
        return
    ref = O.roi_align_one(torch.from_numpy(F_).double(), torch.from_numpy(box), P, FEAT_SCALES[lvl]).double()
    gh, gw, (y0, y1), (x0, x1) = _roi_grid(box, P, FEAT_SCALES[lvl], H, W)
    fmax = float(np.abs(F_[:, y0:y1, x0:x1]).max()) if gh and gw else 0.0
    s = 2.0 ** -22 if precision == "split" else 2.0 ** -24
    bound = ((gh + 2) * (gw + 2) + gh + gw + 4) * 2.0 ** -24 * fmax + s * ref.abs()
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (box.tolist(), lvl, gh, gw, float(err.max()), float((err / bound.clamp_min(1e-30)).max()))
    ratios.append(float((err / bound.clamp_min(1e-30)).max()))


def _feats_of_image(eng, n, i, cache):
    if "maps" not in cache:
        cache["maps"] = [eng.tensor(f"p{l}", n=n) for l in (2, 3, 4, 5)]
    return [np.ascontiguousarray(m[i].transpose(2, 0, 1)).astype(np.float32) for m in cache["maps"]]


def _sample(rng, m, boxes, lv, P, eng_maps_hw, per_image):
    """per_image RoIs with a fixed seed, plus every RoI whose sampling window exceeds the weight table (g > 21: the per-sample
    fallback of roi_align_win_kernel)."""
    pick = set(rng.choice(m, size=min(m, per_image), replace=False).tolist()) if m else set()
    for r in range(m):
        H, W = eng_maps_hw[lv[r]]
        gh, gw, _, _ = _roi_grid(boxes[r], P, FEAT_SCALES[lv[r]], H, W)
        if max(gh, gw) > 21:
            pick.add(r)
    return sorted(pick)


def check_roi_align_box(spec, eng, n, precision, per_image=40, ratios=None):
    """box RoIAlign of sampled proposals (at their oracle level) against the oracle on the engine's own FPN maps."""
    O = _oracle()
    ratios = [] if ratios is None else ratios
    pb, pc = eng.tensor("proposal_boxes", n=n), eng.tensor("proposal_count", n=n)
    PC = pb.shape[1]
    P = spec.box_pooler_resolution
    pooled = eng.tensor("box_pooled", strip_halo=False)        # (NB*PC, P, P, 256)
    rng = np.random.default_rng(0)
    cache = {}
    for i in range(n):
        m = int(pc[i])
        feats_i = _feats_of_image(eng, n, i, cache)
        lv = O.assign_levels(torch.from_numpy(pb[i, :m]), 2, 5).numpy()
        for r in _sample(rng, m, pb[i], lv, P, [f.shape[1:] for f in feats_i], per_image):
            got = torch.from_numpy(pooled[i * PC + r].astype(np.float32)).permute(2, 0, 1)
            _check_pooled(O, feats_i, pb[i, r], lv[r], P, got, precision, ratios)
    return ratios


def check_roi_align_mask(spec, eng, dets, n, precision, per_image=40, ratios=None):
    """mask RoIAlign of the detections (compact entries, image by image) against the oracle on the engine's own FPN maps."""
    O = _oracle()
    ratios = [] if ratios is None else ratios
    dn = eng.tensor("det_boxes_net", n=n)
    mp = eng.tensor("mask_pooled", strip_halo=True)
    P = spec.mask_pooler_resolution
    rng = np.random.default_rng(1)
    cache = {}
    e = 0
    for i, d in enumerate(dets[:n]):
        m = len(d)
        if m == 0:
            continue
        feats_i = _feats_of_image(eng, n, i, cache)
        lv = O.assign_levels(torch.from_numpy(dn[i, :m]), 2, 5).numpy()
        if precision == "fp16":
            pick = [r for r in range(m) if r % 7 == 0]
        else:
            pick = _sample(rng, m, dn[i], lv, P, [f.shape[1:] for f in feats_i], per_image)
        for r in pick:
            got = torch.from_numpy(mp[e + r].astype(np.float32)).permute(2, 0, 1)
            _check_pooled(O, feats_i, dn[i, r], lv[r], P, got, precision, ratios)
        e += m
    return ratios


def check_box_postprocess(spec, eng, dets, n, tile_hw):
    """fast_rcnn_inference_single_image + detector_postprocess on the engine's own box-head output: detection count and
    classes exact, scores 2e-6, boxes 1e-3 px (tile) / 2e-3 px (network input)."""
    O = _oracle()
    K = spec.num_classes
    nh, nw, _, _ = eng.net_shape()
    pred = torch.from_numpy(eng.tensor("box_pred", n=n))
    pb = torch.from_numpy(eng.tensor("proposal_boxes", n=n))
    pc = eng.tensor("proposal_count", n=n)
    dn = eng.tensor("det_boxes_net", n=n)
    for i in range(n):
        m = int(pc[i])
        probs = F.softmax(pred[i, :m, :K + 1], dim=-1)
        dec = O.apply_deltas(pred[i, :m, K + 1:5 * K + 1], pb[i, :m], spec.box_reg_weights, spec.scale_clamp)
        ref = O.fast_rcnn_inference_single_image(spec, dec, probs, (nh, nw), nms_trick=False)
        fin = O.detector_postprocess(ref, (nh, nw), tile_hw[0], tile_hw[1])
        d = dets[i]
        assert len(d) == fin["boxes"].shape[0], f"image {i}: {len(d)} detections vs {fin['boxes'].shape[0]}"
        assert np.array_equal(d.pred_classes, fin["classes"].numpy())
        if len(d):
            assert np.abs(d.scores - fin["scores"].numpy()).max() <= 2e-6
            assert np.abs(d.pred_boxes - fin["boxes"].numpy()).max() <= 1e-3
            assert np.abs(dn[i, :len(d)] - ref["boxes"].numpy()[: len(d)]).max() <= 2e-3


def check_mask_paste(spec, dets, tile_hw, images=None):
    """paste: oracle grid_sample on the engine's own probabilities and boxes; <= 1e-4 of the pixels + 2 differ."""
    O = _oracle()
    for i, d in enumerate(dets):
        if len(d) == 0 or (images is not None and i not in images):
            continue
        ref = O.paste_masks(torch.from_numpy(d.mask_probs)[:, None], torch.from_numpy(d.pred_boxes), tile_hw[0], tile_hw[1],
                            spec.mask_threshold).numpy()
        gm = d.pred_masks
        assert gm.shape == ref.shape
        mism = np.logical_xor(gm, ref).sum()
        assert mism <= 1e-4 * ref.size + 2, f"{mism} pasted-mask pixels differ"


def test_rpn_stage_exact(small):
    spec, W, tiles, eng, _ = small
    check_rpn_stage(spec, eng, 3)


def test_rpn_nms_stage_exact(small):
    spec, W, tiles, eng, _ = small
    assert check_rpn_nms(spec, eng, 3) == "global"


def test_roi_align_box_stage(small):
    spec, W, tiles, eng, _ = small
    check_levels(eng, 3)
    check_roi_align_box(spec, eng, 3, "fp16")


def test_box_head_stage(small):
    spec, W, tiles, eng, _ = small
    O = _oracle()
    W16 = _r16w(W)
    pc = eng.tensor("proposal_count", n=3)
    pooled = eng.tensor("box_pooled", strip_halo=False)
    pred = eng.tensor("box_pred", n=3)
    K = spec.num_classes
    for i in range(3):
        n = int(pc[i])
        x = torch.from_numpy(pooled[i * 1024:i * 1024 + n].astype(np.float32)).permute(0, 3, 1, 2)   # (n,256,7,7)
        _, cls, reg = O.box_head(W16, x)
        got = torch.from_numpy(pred[i, :n])
        # two fp16-rounded hidden layers (1024 wide) in between: 1e-2 absolute on O(1) logits
        assert float((got[:, :K + 1] - cls).abs().max()) <= 1e-2 * max(1.0, float(cls.abs().max()))
        assert float((got[:, K + 1:5 * K + 1] - reg).abs().max()) <= 1e-2 * max(1.0, float(reg.abs().max()))


def test_box_postprocess_stage_exact(small):
    spec, W, tiles, eng, dets = small
    check_box_postprocess(spec, eng, dets, 3, (256, 256))


def test_box_nms_stage_exact(small):
    spec, W, tiles, eng, _ = small
    assert check_box_nms(spec, eng, 3) == "global"


def test_mask_stage(small):
    spec, W, tiles, eng, dets = small
    O = _oracle()
    W16 = _r16w(W)
    total = int(eng.tensor("det_total")[0])
    assert total == sum(len(d) for d in dets)
    mp = eng.tensor("mask_pooled", strip_halo=True)[:total]                  # compact entries
    x = torch.from_numpy(mp.astype(np.float32)).permute(0, 3, 1, 2)
    classes = torch.from_numpy(np.concatenate([d.pred_classes for d in dets]))
    _, probs = O.mask_head(spec, W16, x, classes)
    got = np.concatenate([d.mask_probs for d in dets])
    # 6 fp16-rounded layers before the sigmoid: 2e-2 absolute on probabilities
    assert np.abs(got - probs[:, 0].numpy()).max() <= 2e-2
    check_mask_paste(spec, dets, (256, 256))


def test_mask_roi_align_stage(small):
    spec, W, tiles, eng, dets = small
    check_roi_align_mask(spec, eng, dets, 3, "fp16")


SMALL_SPEC = dict(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300)


def _tie_tiles(h, w):
    """An all-zero tile, a tile with a constant no-data band over 40 % of it, and a synthetic scene."""
    t = synthetic_tiles(3, h, w, 3, seed=91)
    t[0] = 0
    t[1, : int(0.4 * h)] = 0
    return t


# cell -> (precision, spec overrides, batch, tile side, tiles)
STAGE_CELLS = {
    "b_split_default_b16": ("split", {}, 16, 512, "synthetic"),
    "c_split_default_b1_graph": ("split", {}, 1, 512, "synthetic"),
    "d_fp32_small_b7": ("fp32", SMALL_SPEC, 7, 256, "synthetic"),
    "e_fp16_small_k8_b5": ("fp16", dict(SMALL_SPEC, num_classes=8), 5, 256, "synthetic"),
    "f_split_small_k1_ties": ("split", dict(SMALL_SPEC, num_classes=1), 3, 256, "ties"),
}


@pytest.mark.parametrize("cell", list(STAGE_CELLS))
def test_stage_exact_across_configurations(gpu_required, cell):
    """The stage checks of the fp16 `small` tests on the configurations the product runs: the split mode at
    the bench configuration (batch 16: RPN NMS with the mask in LDS over 80 segments, top-k over 120 000 p2 anchors, the
    detection cap) and at batch 1 through the hipGraph replay, the fp32 mode (per-sample roi_align_kernel; 35 RPN segments, LDS),
    fp16 with 8 classes (40 box-NMS segments, LDS; det_merge at its class limit) and the split mode with one class on an
    all-zero tile, a tile with a constant band and a scene, with the objectness weights zeroed so that logits tie exactly: at
    least one (image, level) holds more logits equal to the k-th largest than the top-k takes, and the engine must take the
    lower anchor indices first, as the oracle's stable sort does, through the top-k, the RPN NMS and the merge.  Index work is
    exact; RoIAlign in split / fp32 is held to the bound of its operation order against a float64 oracle."""
    precision, over, n, side, kind = STAGE_CELLS[cell]
    spec = EngineSpec(**over).replace(precision=precision)
    W = synthetic_weights(spec, seed=0)
    if kind == "ties":
        # objectness = its bias alone: every anchor of a type has the same logit in every image and level, so the top-k cut, the
        # RPN NMS and the level merge all decide between equal scores (the random FPN maps alone never tie exactly: every
        # position sees the zero padding of the deep layers)
        W = dict(W)
        k = "proposal_generator.rpn_head.objectness_logits.weight"
        W[k] = W[k] * 0
    tiles = _tie_tiles(side, side) if kind == "ties" else synthetic_tiles(max(n, 3), side, side, 3, seed=101)
    eng = Engine(spec, W, (side, side, 3), max_batch=n)
    try:
        if n == 1:                                     # batch 1: warm-up and graph capture on other tiles, then the replay
            for t in (2, 1):
                eng.infer(tiles[t:t + 1], want_probs=True)
        dets = eng.infer(tiles[:n], want_probs=True)
        if kind == "ties":
            ties = rpn_topk_ties(spec, eng, n)
            assert any(eq > taken for eq, taken in ties.values()), ties
        check_rpn_stage(spec, eng, n)
        rpn_form = check_rpn_nms(spec, eng, n)
        box_form = check_box_nms(spec, eng, n)
        check_levels(eng, n)
        rb = check_roi_align_box(spec, eng, n, precision)
        rm = check_roi_align_mask(spec, eng, dets, n, precision)
        check_box_postprocess(spec, eng, dets, n, (side, side))
        check_mask_paste(spec, dets, (side, side), images=None if n <= 7 else set(range(0, n, 4)))
        print(f"STAGE_CELL {cell}: rpn_nms={rpn_form} ({n * len(spec.rpn_in_features)} segments) box_nms={box_form} "
              f"({n * spec.num_classes} segments) detections={[len(d) for d in dets]} "
              f"roi_box_max_err_over_bound={max(rb) if rb else None} roi_mask_max_err_over_bound={max(rm) if rm else None} "
              f"(box RoIs {len(rb)}, mask RoIs {len(rm)})")
        if spec.num_classes == 8:
            assert box_form == "lds"
    finally:
        eng.close()


def test_end_to_end_small(small):
    spec, W, tiles, eng, dets = small
    O = _oracle()
    m = O.OracleModel(spec, W)
    ref = m([tiles[i] for i in range(3)])
    fracs = []
    for i in range(3):
        r = {"boxes": ref[i]["boxes"].numpy(), "scores": ref[i]["scores"].numpy(), "classes": ref[i]["classes"].numpy(), "masks": ref[i]["masks"].numpy()}
        g = {"boxes": dets[i].pred_boxes, "scores": dets[i].scores, "classes": dets[i].pred_classes, "masks": dets[i].pred_masks}
        fw = match_detections(r, g)
        bw = match_detections(g, r)
        print("end_to_end_small", i, fw, bw)
        fracs += [fw["frac_matched"], bw["frac_matched"]]
        assert fw["max_dscore"] <= 0.02 and fw["min_mask_iou"] >= 0.8 and fw["agg_mask_iou"] >= 0.9, fw
    # random-weight workload: a statistical comparison (module docstring) -- any change of the fp32 summation order moves single
    # tiles by several percent; the stated tolerance is asserted on the trained-like workload and in reference precision
    assert np.mean(fracs) >= 0.85 and min(fracs) >= 0.7, fracs


def test_batch_independence_and_determinism(small):
    """Tiles are independent units: tile i alone == tile i inside a batch, and two runs agree bit for bit."""
    spec, W, tiles, eng, dets = small
    again = eng.infer(tiles, want_probs=True)
    single = eng.infer(tiles[1:2], want_probs=True)[0]
    for a, b in zip(dets, again):
        assert np.array_equal(a.pred_boxes, b.pred_boxes) and np.array_equal(a.scores, b.scores)
        assert np.array_equal(a._packed, b._packed)
    assert np.array_equal(single.pred_boxes, dets[1].pred_boxes)
    assert np.array_equal(single.scores, dets[1].scores)
    assert np.array_equal(single._packed, dets[1]._packed)


@pytest.mark.parametrize("shared", [False, True])
def test_lane_pipeline_equals_single_engine(small, shared):
    """Two-lane pipeline, both forms -- independent lanes (each a whole engine on its own stream; the default) and the phase-interleaved form
    (rs_engine_infer_phase on a shared wide stream, glue on side streams): five batches of different tiles through alternating lanes give
    bit-identical detections to the single engine."""
    from proj_roadsurf_amd.engine import LanePipeline
    spec, W, tiles, eng, _ = small
    batches = [synthetic_tiles(3, 256, 256, 3, seed=500 + k) for k in range(5)]
    want = [eng.infer(b) for b in batches]
    pipe = LanePipeline(spec, W, (256, 256, 3), max_batch=4, lanes=2, shared_stream=shared)
    try:
        assert (pipe.engines[1].stream == pipe.engines[0].stream) == shared
        got = [None] * len(batches)
        prev = None
        for k, b in enumerate(batches):
            lane = pipe.lane_of_next()
            lane_idx = pipe.submit(lane.upload_tiles(b), len(b))
            assert lane_idx == k % 2
            if prev is not None:                       # shared form: batch k-1 is complete once batch k has been submitted (fetch waits for the lane's own work)
                got[prev[0]] = pipe.engines[prev[1]].fetch(3)
            prev = (k, lane_idx)
        pipe.flush()
        got[prev[0]] = pipe.engines[prev[1]].fetch(3)
        for w_b, g_b in zip(want, got):
            for a, b in zip(w_b, g_b):
                assert len(a) == len(b) and len(a) > 0
                assert np.array_equal(a.pred_boxes, b.pred_boxes) and np.array_equal(a.scores, b.scores)
                assert np.array_equal(a.pred_classes, b.pred_classes) and np.array_equal(a._packed, b._packed)
    finally:
        pipe.close()


def test_independent_lanes_are_bit_reproducible_under_load(gpu_required):
    """Two engines on independent streams, fed alternately without waiting (tools/parity/lanes_stress.py in small): 240 tile results, every field against
    the same engine run alone.  Before csrc/common.h rs_fdiv this failed in the packed masks about once per 500 tile results: the compiler's fp32 division
    sequence returns wrong quotients in a wave that shares its SIMD with another kernel's MFMA waves."""
    from proj_roadsurf_amd.engine import LanePipeline
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    B, T = 3, 256
    batches = [synthetic_tiles(B, T, T, 3, seed=700 + k) for k in range(6)]
    solo = Engine(spec, W, (T, T, 3), max_batch=4)
    pipe = LanePipeline(spec, W, (T, T, 3), max_batch=4, lanes=2)
    try:
        want = [solo.infer(b) for b in batches]
        for r in range(20):
            order = [(r + i) % len(batches) for i in range(4)]
            got = []
            for i, bi in enumerate(order):
                e = pipe.engines[i % 2]
                if i >= 2:
                    got.append((order[i - 2], e.fetch(B)))
                e.infer_device(e.upload_tiles(batches[bi]), B)
            got += [(order[2 + i], pipe.engines[i].fetch(B)) for i in range(2)]
            for bi, res in got:
                assert all(_same_instances(a, b) for a, b in zip(want[bi], res)), (r, bi)
    finally:
        pipe.close()
        solo.close()


def test_two_engines_driven_from_two_host_threads(gpu_required):
    """calls on different engines may come from different host threads at the same time (ctypes drops the GIL around every call; the
    library keeps its error text and its last-variant note per thread).  Two threads, each with its own engine, 12 forwards of different batches each,
    every result against the same engine run alone."""
    import threading
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    B, T = 3, 256
    batches = [synthetic_tiles(B, T, T, 3, seed=810 + k) for k in range(4)]
    solo = Engine(spec, W, (T, T, 3), max_batch=4)
    engs = [Engine(spec, W, (T, T, 3), max_batch=4) for _ in range(2)]
    try:
        want = [solo.infer(b) for b in batches]
        errors = []

        def work(ti):
            try:
                for r in range(12):
                    bi = (r + 2 * ti) % len(batches)
                    got = engs[ti].infer(batches[bi])
                    if not all(_same_instances(a, b) for a, b in zip(want[bi], got)):
                        errors.append((ti, r, bi))
            except Exception as ex:          # noqa: BLE001
                errors.append((ti, repr(ex)))
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
    finally:
        for e in engs:
            e.close()
        solo.close()


def test_lane_pipeline_streaming_host_interface(small):
    """LanePipeline.run: host batches in, detections out, `lanes` batches of look-ahead, pinned staging + asynchronous result
    copies (rs_engine_upload_async / fetch_async / fetch_wait) -- same detections as the synchronous single engine, in order,
    including a ragged last batch; independent lanes (two, three), the shared-stream form, and a single lane."""
    from proj_roadsurf_amd.engine import LanePipeline
    spec, W, tiles, eng, _ = small
    batches = [synthetic_tiles(3 if k != 6 else 2, 256, 256, 3, seed=900 + k) for k in range(7)]
    want = [eng.infer(b) for b in batches]
    for lanes, shared in ((2, False), (2, True), (3, False), (1, False)):
        pipe = LanePipeline(spec, W, (256, 256, 3), max_batch=4, lanes=lanes, shared_stream=shared)
        try:
            got = list(pipe.run(iter(batches)))
            assert len(got) == len(want)
            for w_b, g_b in zip(want, got):
                assert len(w_b) == len(g_b)
                for a, b in zip(w_b, g_b):
                    assert len(a) == len(b) and len(a) > 0
                    assert np.array_equal(a.pred_boxes, b.pred_boxes) and np.array_equal(a.scores, b.scores)
                    assert np.array_equal(a.pred_classes, b.pred_classes) and np.array_equal(a._packed, b._packed)
        finally:
            pipe.close()


def test_fp16_meets_the_stated_tolerance_on_a_trained_like_detector(gpu_required):
    """SURVEY.md §8d's tolerance for the fp16 production mode, asserted at its stated values on the workload it is meant for: a
    detector whose scores separate and whose duplicate proposals regress to the same object.  FOUR training campaigns (seeds 0..3 of
    the repo's own training engine, 600 SGD steps each on synthetic scenes with two object classes, ~12 s per campaign; the seeds are
    the first four, not chosen) x 48 fresh 512x512 scenes with 4-12 objects (800x800 network input, 1000 proposals): fp16 engine vs
    fp32 oracle, >= 1500 reference detections pooled.  A detection counts as matched when ALL of section 8d's conditions hold for its
    pair: same class, box IoU >= 0.95, |dscore| <= 0.02, mask IoU >= 0.95 on the pasted 512 x 512 masks (every mask, small ones too).
    Asserted on the POOL, both directions: matched fraction >= 0.98 AND the 95 % Wilson lower bound of it >= 0.98; per scene only
    that the masks of the box-matched pairs overlap >= 0.95 in aggregate (one pair with a mask IoU of 0.90 next to 1 800 good ones is a
    miss of the pool, not a failure).  Since round 3 the training runs are bit-reproducible (owner-computes RoIAlign backward,
    tests/test_gpu_trainer.py::test_two_training_runs_give_the_same_bits), so this pool is the same from run to run.
    Measured (round 3, profiles/r03/parity/): 99.3-99.7 % matched, lower bound 0.989+; the residual misses are near-ties of two boxes
    of ONE object in the final NMS (scores 1e-4 apart, IoU 0.7-0.9 between them) which the fp16 trunk's 4e-4 feature noise flips --
    tools/parity/bisect_stages.py finds 11 of 15 such scenes (8 seeds) already in "oracle downstream of the engine's FPN maps", 4 created
    by the RPN's 3x3 convolution, none by any later stage."""
    from proj_roadsurf_amd.matching import wilson_lower
    from proj_roadsurf_amd.synthetic import synthetic_scenes, train_trained_like
    from tests.util import box_iou
    O = _oracle()
    spec = EngineSpec(num_classes=2)
    n, B = 48, 16
    tot = {"fw_n": 0, "fw_m": 0, "bw_n": 0, "bw_m": 0}
    for seed in (0, 1, 2, 3):
        W, curve = train_trained_like(spec, 512, steps=600, seed=seed)
        assert np.mean(curve[-20:]) < 0.6 * curve[0], (seed, curve[0], np.mean(curve[-20:]))          # it did train
        tiles, gtb, gtc, _ = synthetic_scenes(n, 512, 512, 3, seed=987654 + seed, objects=(4, 12))
        eng = Engine(spec, W, (512, 512, 3), max_batch=B)
        try:
            dets = [d for b0 in range(0, n, B) for d in eng.infer(tiles[b0:b0 + B])]
        finally:
            eng.close()
        m = O.OracleModel(spec, W)
        st = {"fw_n": 0, "fw_m": 0, "bw_n": 0, "bw_m": 0}
        recalled = total_gt = 0
        for i in range(n):
            ref = m([tiles[i]])[0]
            r = {"boxes": ref["boxes"].numpy(), "scores": ref["scores"].numpy(), "classes": ref["classes"].numpy(), "masks": ref["masks"].numpy()}
            g = {"boxes": dets[i].pred_boxes, "scores": dets[i].scores, "classes": dets[i].pred_classes, "masks": dets[i].pred_masks}
            fw, bw = match_detections(r, g), match_detections(g, r)
            for t in (tot, st):
                t["fw_n"] += fw["n_ref"]; t["fw_m"] += fw["n_full"]; t["fw_box"] = t.get("fw_box", 0) + fw["n_matched"]
                t["bw_n"] += bw["n_ref"]; t["bw_m"] += bw["n_full"]; t["bw_box"] = t.get("bw_box", 0) + bw["n_matched"]
            assert fw["agg_mask_iou"] >= 0.95, (seed, i, fw)
            hi = dets[i].scores >= 0.5
            iou = box_iou(gtb[i], dets[i].pred_boxes[hi]) if hi.any() else np.zeros((len(gtb[i]), 0))
            recalled += int((iou.max(1) >= 0.5).sum()) if iou.shape[1] else 0
            total_gt += len(gtb[i])
        print("trained_like seed", seed, st, "gt recalled", recalled, "of", total_gt, "loss", round(float(np.mean(curve[-20:])), 3))
        assert recalled >= 0.9 * total_gt, "the trained-like detector does not detect its objects"
    lo_fw, lo_bw = wilson_lower(tot["fw_m"], tot["fw_n"]), wilson_lower(tot["bw_m"], tot["bw_n"])
    print("trained_like pooled", tot, "matched", round(tot["fw_m"] / tot["fw_n"], 4), round(tot["bw_m"] / tot["bw_n"], 4),
          "Wilson 95 % lower bound", round(lo_fw, 4), round(lo_bw, 4))
    assert tot["fw_n"] >= 1500
    assert tot["fw_m"] >= 0.98 * tot["fw_n"] and tot["bw_m"] >= 0.98 * tot["bw_n"], tot
    assert lo_fw >= 0.98 and lo_bw >= 0.98, (tot, lo_fw, lo_bw)


def test_full_size_512_tile(gpu_required):
    """BASELINE config 1/2 geometry: 512x512x3 tiles -> 800x800 network input, 1000 proposals, 100 detections.
    fp16 production mode vs fp32 oracle is a STATISTICAL comparison on this random-weight workload (a single
    flipped NMS decision cascades), so it is evaluated over 3 tiles: mean matched fraction >= 0.85, no tile
    below 0.7; scores of matched pairs agree to 2e-2 (measured: 1e-3).  The strict end-to-end check is the
    fp32 validation mode below."""
    O = _oracle()
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 512, 512, 3, seed=1234)
    eng = Engine(spec, W, (512, 512, 3), max_batch=3)
    try:
        assert eng.net_shape() == (800, 800, 800, 800)
        dets = eng.infer(tiles)
        m = O.OracleModel(spec, W)
        fracs = []
        for i in range(3):
            ref = m([tiles[i]])[0]
            r = {"boxes": ref["boxes"].numpy(), "scores": ref["scores"].numpy(), "classes": ref["classes"].numpy(), "masks": ref["masks"].numpy()}
            g = {"boxes": dets[i].pred_boxes, "scores": dets[i].scores, "classes": dets[i].pred_classes, "masks": dets[i].pred_masks}
            fw = match_detections(r, g)
            bw = match_detections(g, r)
            print("full_size_512", i, fw, bw)
            assert fw["n_ref"] > 0
            assert fw["max_dscore"] <= 0.02 and fw["agg_mask_iou"] >= 0.9, fw
            fracs += [fw["frac_matched"], bw["frac_matched"]]
        assert np.mean(fracs) >= 0.85 and min(fracs) >= 0.7, fracs
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# fp32 validation mode (rs_spec.precision = 1): every conv/linear layer in plain fp32.  Here the
# SURVEY.md §8d "fp32 validation" bar applies end to end against the fp32 oracle:
# >= 98 % of detections matched both ways, |dbox| <= 1e-2 px, |dscore| <= 1e-4 on matched pairs.
# ---------------------------------------------------------------------------------------------
def _strict_compare(ref, det, tag):
    r = {"boxes": ref["boxes"].numpy(), "scores": ref["scores"].numpy(), "classes": ref["classes"].numpy(), "masks": ref["masks"].numpy()}
    g = {"boxes": det.pred_boxes, "scores": det.scores, "classes": det.pred_classes, "masks": det.pred_masks}
    fw, bw = match_detections(r, g, min_score=0.05, iou_thr=0.99), match_detections(g, r, min_score=0.05, iou_thr=0.99)
    print(tag, fw, bw)
    assert fw["frac_matched"] >= 0.98 and bw["frac_matched"] >= 0.98, (fw, bw)
    assert fw["max_dscore"] <= 1e-4, fw
    assert fw["agg_mask_iou"] >= 0.995, fw
    assert fw["max_dbox"] <= 1e-2, fw          # matched pairs (two detections with scores 1e-6 apart may swap rank)


# Both reference-precision modes are held to the same bounds: "fp32" = fp32 operands on the fp32 matrix cores (csrc/ref_f32.hip), "split" = hi + lo
# fp16 operand planes, three products on the fp16 matrix cores (csrc/common.h ConvParams::split; operator tests in tests/test_gpu_split.py).
REF_MODES = ["fp32", "split"]


def _net_input_equal(x, want, precision):
    """fp32 mode: bit-exact.  split mode: the fp32 value to the 22 significand bits its two planes hold."""
    if precision == "split":
        return bool(np.abs(x - want).max() <= 2.0 ** -22 * np.abs(want).max())
    return np.array_equal(x, want)


@pytest.mark.parametrize("precision", REF_MODES)
def test_fp32_mode_end_to_end_small(gpu_required, precision):
    O = _oracle()
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                      precision=precision)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    eng = Engine(spec, W, (256, 256, 3), max_batch=3)
    try:
        dets = eng.infer(tiles)
        feats = O.OracleModel(spec, W)
        ref = feats([tiles[i] for i in range(3)], keep=True)
        # backbone maps now agree to fp32 rounding
        for name in ["res2", "res5", "p2", "p6"]:
            got = torch.from_numpy(eng.tensor(name, n=3)).permute(0, 3, 1, 2)
            want = torch.stack([ref[i]["inter"]["feats"][name] for i in range(3)])
            rel = float((got - want).norm() / want.norm())
            assert rel <= 2e-5, f"{name}: rel L2 err {rel}"
        for i in range(3):
            _strict_compare(ref[i], dets[i], f"fp32_small[{i}]")
    finally:
        eng.close()


@pytest.mark.parametrize("precision", REF_MODES)
def test_fp32_mode_full_size_tile(gpu_required, precision):
    O = _oracle()
    spec = EngineSpec(num_classes=2, precision=precision)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(1, 512, 512, 3, seed=1234)
    eng = Engine(spec, W, (512, 512, 3), max_batch=1)
    try:
        dets = eng.infer(tiles)
        ref = O.OracleModel(spec, W)([tiles[0]])
        _strict_compare(ref[0], dets[0], "fp32_full")
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# Other configurations of the boundary: 4-band tiles that are DOWN-scaled (BASELINE configs[3] geometry,
# reduced), non-square tiles with size-divisibility padding, and the YAML's own NUM_CLASSES = 1.
# All in fp32 validation mode so that the comparison with the oracle is strict.
# ---------------------------------------------------------------------------------------------
def _run_strict(spec, tiles, tag):
    O = _oracle()
    W = synthetic_weights(spec, seed=0)
    eng = Engine(spec, W, tiles.shape[1:], max_batch=tiles.shape[0])
    try:
        dets = eng.infer(tiles)
        ref = O.OracleModel(spec, W)([tiles[i] for i in range(tiles.shape[0])], keep=True)
        x = eng.tensor("net_input", n=tiles.shape[0])
        for i in range(tiles.shape[0]):
            want = ref[i]["inter"]["net_input"].permute(1, 2, 0).numpy()
            c = want.shape[2]
            assert _net_input_equal(x[i, :, :, :c], want, spec.precision), f"{tag}: pre-processing differs"
            _strict_compare(ref[i], dets[i], f"{tag}[{i}]")
        return eng.net_shape()
    finally:
        eng.close()


@pytest.mark.parametrize("precision", REF_MODES)
def test_fp32_mode_4band_downscaled_tiles(gpu_required, precision):
    """RGB+NIR tiles, 400x400 -> 320x320: Pillow's antialiased down-scaling path, 4 input channels,
    channel reversal of all 4 bands (what `im[:, :, ::-1]` does in DefaultPredictor)."""
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                      pixel_mean=(103.53, 116.28, 123.675, 110.0), pixel_std=(1.0, 1.0, 1.0, 1.0), precision=precision)
    tiles = synthetic_tiles(2, 400, 400, 4, seed=31)
    assert _run_strict(spec, tiles, "4band") == (320, 320, 320, 320)


@pytest.mark.parametrize("precision", REF_MODES)
def test_fp32_mode_non_square_tile_with_padding(gpu_required, precision):
    """200x300 tile -> ResizeShortestEdge gives 224x336, padded to 224x352 (size_divisibility 32): the padded
    columns are zeros at the network input but real pixels from the stem on."""
    spec = EngineSpec(num_classes=2, min_size_test=224, max_size_test=400, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200,
                      precision=precision)
    tiles = synthetic_tiles(2, 200, 300, 3, seed=41)
    assert _run_strict(spec, tiles, "nonsquare") == (224, 336, 224, 352)


@pytest.mark.parametrize("precision", REF_MODES)
def test_fp32_mode_single_class(gpu_required, precision):
    """ROI_HEADS.NUM_CLASSES = 1 as written in the reference YAML (R:config/detectron2_config_3bands.yaml:191)."""
    spec = EngineSpec(num_classes=1, min_size_test=256, max_size_test=426, rpn_pre_nms_topk_test=200, rpn_post_nms_topk_test=200,
                      precision=precision)
    tiles = synthetic_tiles(2, 192, 192, 3, seed=51)
    _run_strict(spec, tiles, "k1")


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_no_detections_and_mixed_batches(gpu_required, precision):
    """Edge cases of the detection bookkeeping: a score threshold nothing passes (zero detections on every tile: the mask head's
    GEMMs run over a device-side count of 0), then a batch in which only SOME tiles have detections (compacted mask-head list with
    empty images in the middle), each compared with the same tile run alone.  In the fp16 and in the split-operand mode (other kernels
    behind the mask head's device-side row count)."""
    spec_hi = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300,
                         score_thresh_test=0.9999, precision=precision)
    W = synthetic_weights(spec_hi, seed=0)
    tiles = synthetic_tiles(3, 256, 256, 3, seed=77)
    eng = Engine(spec_hi, W, (256, 256, 3), max_batch=4)
    try:
        out = eng.infer(tiles)
        assert [len(o) for o in out] == [0, 0, 0]
        for o in out:
            assert o.pred_boxes.shape == (0, 4) and o.scores.shape == (0,) and o.pred_classes.shape == (0,)
            assert o.pred_masks.shape == (0, 256, 256)
        assert [len(o) for o in eng.infer(tiles[:1])] == [0]                       # and the engine is still usable
    finally:
        eng.close()
    # a threshold between the tiles' best scores: some images keep detections, others none
    spec = EngineSpec(num_classes=2, min_size_test=320, max_size_test=533, rpn_pre_nms_topk_test=300, rpn_post_nms_topk_test=300, precision=precision)
    eng = Engine(spec, W, (256, 256, 3), max_batch=4)
    try:
        best = sorted(float(o.scores.max()) for o in eng.infer(tiles))
    finally:
        eng.close()
    thr = 0.5 * (best[0] + best[1]) if best[1] > best[0] else best[0] * 0.999
    spec_mid = spec.replace(score_thresh_test=float(thr))
    eng = Engine(spec_mid, W, (256, 256, 3), max_batch=4)
    try:
        batch = eng.infer(tiles)
        counts = [len(o) for o in batch]
        assert min(counts) == 0 or best[1] == best[0]
        assert max(counts) > 0
        for i in range(3):
            alone = eng.infer(tiles[i:i + 1])[0]
            assert len(alone) == counts[i]
            assert np.array_equal(alone.pred_boxes, batch[i].pred_boxes) and np.array_equal(alone.scores, batch[i].scores)
            assert np.array_equal(alone._packed, batch[i]._packed)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# The configurations bench.py measures (BASELINE.json configs[1] and configs[3]) at full size.  The conv tile variant is
# chosen from M = batch * pixels (csrc/conv_igemm.hip conv_choose_variant), so batch 16 / batch 8 launch other kernels than
# the batch 1-3 tests above; every variant accumulates each output over K in the same order, so a tile's result must not
# depend on the batch it travels in.
# ---------------------------------------------------------------------------------------------
def _same_instances(a, b):
    return (len(a) == len(b) and np.array_equal(a.pred_boxes, b.pred_boxes) and np.array_equal(a.scores, b.scores) and
            np.array_equal(a.pred_classes, b.pred_classes) and np.array_equal(a._packed, b._packed))


def test_engine_launches_the_tabled_variants(gpu_required):
    """What the engine launches per layer at batch 1 / 3 / 8 / 16 of the 800x800 input == the committed dispatch table
    (tests/golden/conv_variants.json, whose CPU side is tests/test_host_cpu.py::test_conv_variant_table)."""
    import json
    import os
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_variants.json")))
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(16, 512, 512, 3, seed=1234)
    eng = Engine(spec, W, (512, 512, 3), max_batch=16)
    try:
        for bi, b in enumerate(gold["batches"]):
            eng.infer(tiles[:b])
            got = eng.stage_variants()
            assert list(got) == list(gold["variants"]), "stage list changed: regenerate tests/golden/conv_variants.json"
            for name, v in got.items():
                assert v == gold["variants"][name][bi], f"batch {b}, {name}: launched variant {v}, table says {gold['variants'][name][bi]}"
    finally:
        eng.close()


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_fused_stem_changes_no_bit(gpu_required, monkeypatch, precision):
    """conv 7x7 s2 + ReLU + max-pool in one launch (csrc/stem_fused.hip: conv outputs of an 8x8 pooled patch kept in LDS) against the
    stand-alone stem conv followed by the pooling kernel (RS_FUSE_STEM=0): the pooled map and the detections are bit-identical -- same
    MFMA K order, same fp16 rounding before the max (split mode: the same three passes over K, the same (hi, lo) pair per value).  3-band and 4-band tiles, up- and down-scaling, a non-square input."""
    for shape, kw in (((512, 512, 3), {}), ((1024, 1024, 4), {}), ((300, 420, 3), dict(min_size_test=320, max_size_test=533))):
        spec = EngineSpec(num_classes=2, precision=precision, **kw)
        if shape[2] == 4:
            spec = spec.replace(pixel_mean=(103.53, 116.28, 123.675, 110.0), pixel_std=(1.0, 1.0, 1.0, 1.0))
        W = synthetic_weights(spec, seed=0)
        tiles = synthetic_tiles(2, *shape, seed=11)
        outs = []
        for env in ("1", "0"):
            monkeypatch.setenv("RS_FUSE_STEM", env)
            eng = Engine(spec, W, shape, max_batch=2)
            try:
                dets = eng.infer(tiles)
                outs.append((dets, eng.tensor("stem").copy(), list(eng.stage_variants())))      # split mode: fp32(hi) + fp32(lo), exact and one-to-one
            finally:
                eng.close()
        (d1, s1, n1), (d0, s0, n0) = outs
        assert "stem.conv1+maxpool" in n1 and "stem.conv1" in n0
        assert float(np.abs(s1.astype(np.float32)).max()) > 0 and np.array_equal(s1, s0), shape
        assert all(_same_instances(a, b) for a, b in zip(d0, d1))


def test_roi_visiting_order_is_a_permutation_and_changes_no_bit(gpu_required, monkeypatch):
    """box.roi_align visits the proposals sorted by (pooler level, top row, left column) instead of in score order, so that
    neighbouring workgroups read neighbouring rows of one feature map (L2 hits; csrc/detect_kernels.hip rpn_merge_kernel, csrc/roi_align.hip /
    RoiAlignParams::order).  Pure scheduling: the order is a permutation of every image's slots, sorted as stated over the valid
    ones, and the pooled features, levels and detections are BIT-identical to the engine without it (RS_ROI_ORDER=0)."""
    spec = EngineSpec(num_classes=2, min_size_test=512, max_size_test=853)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 512, 512, 3, seed=99)
    O = _oracle()

    def run(want_order):
        eng = Engine(spec, W, (512, 512, 3), max_batch=3)
        try:
            dets = eng.infer(tiles)
            out = {n: eng.tensor(n, n=3).copy() for n in ("proposal_boxes", "proposal_count", "box_roi_level")}
            out["box_pooled"] = eng.tensor("box_pooled", strip_halo=False)[:3 * 1024].copy()
            assert ("proposal_order" in eng.tensor_names()) == want_order
            if want_order:
                out["order"] = eng.tensor("proposal_order", n=3).copy()
            return dets, out
        finally:
            eng.close()
    d1, t1 = run(True)
    monkeypatch.setenv("RS_ROI_ORDER", "0")
    d0, t0 = run(False)
    for k in ("proposal_boxes", "proposal_count", "box_roi_level", "box_pooled"):
        assert np.array_equal(t0[k], t1[k]), k
    assert float(np.abs(t1["box_pooled"].astype(np.float32)).max()) > 0
    assert all(_same_instances(a, b) for a, b in zip(d0, d1)) and all(len(d) > 0 for d in d1)
    for i in range(3):
        o = t1["order"][i] - i * 1024
        assert sorted(o.tolist()) == list(range(1024)), "not a permutation of the image's slots"
        c = int(t1["proposal_count"][i])
        assert c > 100 and sorted(o[:c].tolist()) == list(range(c)), "valid slots first"
        b = t1["proposal_boxes"][i][o[:c]]
        lv = O.assign_levels(torch.from_numpy(b), 2, 5).numpy()
        key = lv.astype(np.int64) * (1 << 26) + np.minimum(np.floor(np.maximum(b[:, 1], 0)), 8191).astype(np.int64) * (1 << 13) + \
            np.minimum(np.floor(np.maximum(b[:, 0], 0)), 8191).astype(np.int64)
        assert np.all(np.diff(key) >= 0), "valid slots are not sorted by (level, row, column)"


def test_merged_level_launches_and_split_tail_change_no_bit(gpu_required, monkeypatch):
    """The FPN output convolutions of p2..p5 and the shared RPN 3x3 over p2..p6 run as one multi-map conv_deep launch each, and
    a last round that fills at most half the chip runs as 128-pixel tiles (csrc/conv_deep.hip).  Neither changes the arithmetic
    of any output element: every FPN map, every RPN head output and the detections are BIT-identical to the engine built with
    per-level launches and whole tiles (RS_MERGE_LEVELS=0, RS_DEEP_TAIL=0).  The RPN heads computed inside the epilogue of the
    merged 3x3 launch (default) sum the same products in another order: fp32 head outputs equal to ~1e-6 of their scale."""
    spec = EngineSpec(num_classes=2, min_size_test=512, max_size_test=853)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(3, 512, 512, 3, seed=4321)
    names = [f"p{l}" for l in range(2, 7)] + [f"rpn_head{l}" for l in range(2, 7)]

    def run():
        eng = Engine(spec, W, (512, 512, 3), max_batch=3)
        try:
            dets = eng.infer(tiles)
            stages = list(eng.stage_variants())
            return dets, {n: eng.tensor(n).copy() for n in names}, stages
        finally:
            eng.close()
    df, tf, sf = run()                                         # shipped configuration
    assert "fpn_output2-5" in sf and "rpn.conv+heads2-6" in sf and not any(s.startswith("rpn.heads") for s in sf)
    monkeypatch.setenv("RS_FUSE_RPN_HEADS", "0")
    d1, t1, s1 = run()
    assert "rpn.conv2-6" in s1 and "rpn.heads2" in s1 and "rpn.conv3" not in s1
    monkeypatch.setenv("RS_MERGE_LEVELS", "0")
    monkeypatch.setenv("RS_DEEP_TAIL", "0")
    d0, t0, s0 = run()
    assert "fpn_output2" in s0 and "rpn.conv6" in s0 and "rpn.conv2-6" not in s0
    for n in names:
        assert np.array_equal(t0[n], t1[n]), n
        assert float(np.abs(t1[n]).max()) > 0
        if n.startswith("p"):
            assert np.array_equal(tf[n], t1[n]), n
        else:
            A5 = 5 * spec.num_anchors
            err = float(np.abs(tf[n][..., :A5] - t1[n][..., :A5]).max())
            assert err <= 2e-5 * max(1.0, float(np.abs(t1[n]).max())), (n, err)
    assert all(_same_instances(a, b) for a, b in zip(d0, d1)) and all(len(d) > 0 for d in d1)
    for a, b in zip(df, d1):                                   # the fused heads move logits by ~1e-6: (nearly) the same detections
        r = match_detections({"boxes": b.pred_boxes, "scores": b.scores, "classes": b.pred_classes},
                              {"boxes": a.pred_boxes, "scores": a.scores, "classes": a.pred_classes}, iou_thr=0.9)
        assert r["frac_matched"] >= 0.9, r


def test_mask_predictor_in_the_register_weight_kernel_changes_no_bit(gpu_required, monkeypatch):
    """The mask head's deconv + ReLU + predictor runs in conv_wreg.hip (EPI 3: persistent workgroups, one (dy, dx) group's 256 x 256
    weights in registers, the rows bounded by the device-side detection count) instead of conv_igemm's 128 x 256 tile
    (RS_DECONV_VARIANT=14).  Same per-lane dot order, same shuffles, same order over the channel waves: the mask logits and the
    pasted masks are BIT-identical, on a full batch and on a batch whose detections do not fill a tile."""
    spec = EngineSpec(num_classes=2, min_size_test=512, max_size_test=853)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(5, 512, 512, 3, seed=777)

    def run(n):
        eng = Engine(spec, W, (512, 512, 3), max_batch=5)
        try:
            dets = eng.infer(tiles[:n])
            return dets, eng.tensor("mask_probs").copy(), dict(eng.stage_variants())
        finally:
            eng.close()
    for n in (5, 1):
        d1, p1, v1 = run(n)
        assert v1["mask.deconv_predict"] == 22
        monkeypatch.setenv("RS_DECONV_VARIANT", "14")
        d0, p0, v0 = run(n)
        monkeypatch.delenv("RS_DECONV_VARIANT")
        assert v0["mask.deconv_predict"] == 14
        assert float(np.abs(p0).max()) > 0 and np.array_equal(p0, p1), f"batch {n}: {int((p0 != p1).sum())} mask probabilities differ"
        assert all(_same_instances(a, b) for a, b in zip(d0, d1)) and all(len(d) > 0 for d in d1)


def test_every_batch_size_gives_the_same_detections(gpu_required):
    """The tile dispatch, the split last round of conv_deep, the multi-map launches and the tile heights all depend on the batch
    size.  Every batch size from 1 to 16 must give each tile the detections it gets alone, bit for bit."""
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(16, 512, 512, 3, seed=2468)
    eng = Engine(spec, W, (512, 512, 3), max_batch=16)
    try:
        alone = [eng.infer(tiles[i:i + 1])[0] for i in range(16)]
        assert all(len(d) > 0 for d in alone)
        for b in range(2, 17):
            got = eng.infer(tiles[:b])
            for i in range(b):
                assert _same_instances(alone[i], got[i]), f"batch {b}: tile {i} differs from the tile run alone"
    finally:
        eng.close()


def test_config1_batch16_of_512_tiles(gpu_required):
    """BASELINE configs[1], the headline: batch 16 of 512x512x3 tiles, 800x800 network input.
    (a) fp16 production mode: each of the 16 detection sets is BIT-IDENTICAL to the same tile run alone (other tile variants);
    (b) reference-precision mode: batch 16 == the same tiles run alone, bit for bit, and tiles 0 and 15 meet the strict
        bar against the fp32 oracle (>= 98 % matched both ways at IoU >= 0.99, |dscore| <= 1e-4, |dbox| <= 1e-2 px)."""
    O = _oracle()
    spec = EngineSpec(num_classes=2)
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(16, 512, 512, 3, seed=1234)
    eng = Engine(spec, W, (512, 512, 3), max_batch=16)
    try:
        batch = eng.infer(tiles)
        assert all(len(d) > 0 for d in batch)
        for i in (0, 5, 10, 15):
            alone = eng.infer(tiles[i:i + 1])[0]
            assert _same_instances(alone, batch[i]), f"fp16: tile {i} differs between batch 16 and batch 1"
    finally:
        eng.close()
    ref = O.OracleModel(spec, W)([tiles[0], tiles[15]])
    for precision in REF_MODES:
        eng = Engine(spec.replace(precision=precision), W, (512, 512, 3), max_batch=16)
        try:
            batch = eng.infer(tiles)
            for i in (0, 15):
                alone = eng.infer(tiles[i:i + 1])[0]
                assert _same_instances(alone, batch[i]), f"{precision}: tile {i} differs between batch 16 and batch 1"
            _strict_compare(ref[0], batch[0], f"config1_b16[0] {precision}")
            _strict_compare(ref[1], batch[15], f"config1_b16[15] {precision}")
        finally:
            eng.close()


def test_config3_4band_1024_tiles_batch8(gpu_required):
    """BASELINE configs[3] at FULL size: RGB+NIR 1024x1024 tiles (antialiased Pillow down-scaling to 800x800, stem Cin = 4),
    batch 8.  Reference-precision mode: tile 0 meets the strict bar against the oracle; fp16 mode: batch 8 is bit-identical to
    the tiles run alone, pre-processing is bit-exact, and the detections match the oracle's to the fp16 bar of this
    random-weight workload."""
    O = _oracle()
    spec = EngineSpec(num_classes=2, pixel_mean=(103.53, 116.28, 123.675, 110.0), pixel_std=(1.0, 1.0, 1.0, 1.0))
    W = synthetic_weights(spec, seed=0)
    tiles = synthetic_tiles(8, 1024, 1024, 4, seed=4321)
    ref = O.OracleModel(spec, W)([tiles[0]], keep=True)[0]
    for precision in REF_MODES:
        eng = Engine(spec.replace(precision=precision), W, (1024, 1024, 4), max_batch=1)
        try:
            d32 = eng.infer(tiles[:1])[0]
            x = eng.tensor("net_input", n=1)
            assert _net_input_equal(x[0], ref["inter"]["net_input"].permute(1, 2, 0).numpy(), precision), "4-band antialiased resize differs"
            _strict_compare(ref, d32, f"config3_{precision}")
        finally:
            eng.close()
    eng = Engine(spec, W, (1024, 1024, 4), max_batch=8)
    try:
        assert eng.net_shape() == (800, 800, 800, 800)
        batch = eng.infer(tiles)
        for i in (0, 7):
            assert _same_instances(eng.infer(tiles[i:i + 1])[0], batch[i]), f"tile {i} differs between batch 8 and batch 1"
        r = {"boxes": ref["boxes"].numpy(), "scores": ref["scores"].numpy(), "classes": ref["classes"].numpy(), "masks": ref["masks"].numpy()}
        g = {"boxes": batch[0].pred_boxes, "scores": batch[0].scores, "classes": batch[0].pred_classes, "masks": batch[0].pred_masks}
        fw, bw = match_detections(r, g), match_detections(g, r)
        print("config3_fp16", fw, bw)
        assert fw["max_dscore"] <= 0.02 and fw["agg_mask_iou"] >= 0.9, fw
        assert fw["frac_matched"] >= 0.8 and bw["frac_matched"] >= 0.8, (fw, bw)
    finally:
        eng.close()


_GRAPH_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from proj_roadsurf_amd.engine import Engine
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import synthetic_weights
from tests.util import synthetic_tiles
spec = EngineSpec(precision=sys.argv[2])
tiles = synthetic_tiles(4, 512, 512, 3, seed=4242)
eng = Engine(spec, synthetic_weights(spec, seed=0), (512, 512, 3), max_batch=1)
out = {}
for k in range(4):                        # warm-up, capture, replay, replay -- each on a different tile
    d = eng.infer(tiles[k:k + 1], want_probs=True)[0]
    out.update({f"boxes{k}": d.pred_boxes, f"scores{k}": d.scores, f"classes{k}": d.pred_classes, f"packed{k}": d._packed,
                f"probs{k}": d.mask_probs})
eng.close()
np.savez(sys.argv[3], **out)
"""


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_graph_replay_equals_eager_masks_included(gpu_required, tmp_path, precision):
    """Single-tile forwards at the default 512 x 512 spec through the captured hipGraph (RS_GRAPH_SMALL=1) and eagerly (=0), in
    separate processes: boxes, scores, classes, mask probabilities and the packed masks of every forward -- warm-up, capture and
    two replays, each on another tile -- are bit-identical."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for g in ("1", "0"):
        path = str(tmp_path / f"graph{g}.npz")
        p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD, root, precision, path], env=dict(os.environ, RS_GRAPH_SMALL=g),
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        res[g] = dict(np.load(path))
    assert res["1"].keys() == res["0"].keys()
    assert sum(len(res["1"][f"boxes{k}"]) for k in range(4)) > 0
    for key in res["1"]:
        assert res["1"][key].dtype == res["0"][key].dtype and np.array_equal(res["1"][key], res["0"][key]), key
