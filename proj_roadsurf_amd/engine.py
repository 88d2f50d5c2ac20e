"""ctypes binding of ``librs_engine.so`` (C ABI: ``include/rs_engine.h``).

This is the host-side mirror of the call the reference's detector makes per tile,
``DefaultPredictor(cfg)(im)`` ([EXT d2: engine/defaults.py], invoked by the object-detector's
``make_detections.py``, R:README.md:78).  There is no CPU fallback: if the shared library or a HIP
device is missing the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import weakref
import math
import os
import time
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .spec import BATCHED_NMS_MODES, EngineSpec
from .weights import pack_weights

_LIB: Optional[C.CDLL] = None
# RS_ENGINE_LIB: another build of the library (diagnostic builds of tools/ubench: ablations, clock probes); default = the in-tree one
LIB_PATH = os.environ.get("RS_ENGINE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "librs_engine.so")
MAX_LEVELS, MAX_ANCHORS, MASK_SIDE = 5, 8, 28
DT_NP = {1: np.float16, 2: np.float32, 3: np.int32, 4: np.uint8, 5: np.float16}       # 5: two fp16 planes (split-operand mode), value = hi + lo
DT_SPLIT16 = 5


class RsError(RuntimeError):
    pass


class RsSaturationError(RsError):
    """``Predictor(on_saturation="raise")``: a batch had activations clamped to the fp16 range.
    ``saturation`` holds the batch's non-zero counts by stage."""

    def __init__(self, message: str, saturation: Dict[str, int]):
        super().__init__(message)
        self.saturation = saturation


class SaturationWarning(RuntimeWarning):
    """``Predictor(on_saturation="warn")``, the default: a batch had activations clamped to the fp16 range."""


def saturation_message(what: str, sat: Dict[str, int], top: int = 3) -> str:
    """One line: the elements clamped to the fp16 range in ``what`` and the ``top`` stages with the largest counts."""
    worst = sorted(sat.items(), key=lambda kv: -kv[1])[:top]
    return (f"{what}: {sum(sat.values())} activations clamped to the fp16 range (+-65504) in {len(sat)} stage(s), largest: "
            + ", ".join(f"{k} {v}" for k, v in worst) + " -- results may be wrong; precision='fp32' stores fp32 and never clamps")


class RsSpec(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("in_channels", C.c_int32), ("flip_channels", C.c_int32),
        ("pixel_mean", C.c_float * 4), ("pixel_std", C.c_float * 4),
        ("min_size_test", C.c_int32), ("max_size_test", C.c_int32), ("size_divisibility", C.c_int32),
        ("res_blocks", C.c_int32 * 4), ("stem_out_channels", C.c_int32), ("res2_out_channels", C.c_int32),
        ("stride_in_1x1", C.c_int32), ("fpn_out_channels", C.c_int32),
        ("num_levels", C.c_int32), ("num_anchors", C.c_int32),
        ("cell_anchors", ((C.c_float * 4) * MAX_ANCHORS) * MAX_LEVELS), ("anchor_offset", C.c_float),
        ("rpn_bbox_reg_weights", C.c_float * 4), ("rpn_pre_nms_topk", C.c_int32), ("rpn_post_nms_topk", C.c_int32),
        ("rpn_nms_thresh", C.c_float), ("rpn_min_size", C.c_float),
        ("num_classes", C.c_int32), ("box_reg_weights", C.c_float * 4),
        ("score_thresh_test", C.c_float), ("nms_thresh_test", C.c_float), ("detections_per_image", C.c_int32),
        ("box_fc_dim", C.c_int32), ("box_pooler_resolution", C.c_int32),
        ("mask_on", C.c_int32), ("mask_pooler_resolution", C.c_int32), ("mask_num_conv", C.c_int32),
        ("mask_conv_dim", C.c_int32), ("mask_threshold", C.c_float), ("scale_clamp", C.c_float),
        ("precision", C.c_int32), ("batched_nms", C.c_int32),
    ]


# sizeof(rs_spec) before batched_nms was appended (RS_SPEC_SIZE_V1): the library still accepts it and reads the mode as 0
RS_SPEC_SIZE_V1 = RsSpec.batched_nms.offset


class RsDets(C.Structure):
    _fields_ = [("count", C.POINTER(C.c_int32)), ("boxes", C.POINTER(C.c_float)), ("scores", C.POINTER(C.c_float)),
                ("classes", C.POINTER(C.c_int32)), ("masks", C.POINTER(C.c_uint8)), ("mask_probs", C.POINTER(C.c_float))]


class RsMaskCrops(C.Structure):
    _fields_ = [("rects", C.POINTER(C.c_int32)), ("offsets", C.POINTER(C.c_uint32)), ("data", C.POINTER(C.c_uint8)),
                ("capacity", C.c_uint64), ("used", C.c_uint64)]


class RsPolygons(C.Structure):
    _fields_ = [("header", C.POINTER(C.c_int32)), ("poly_ring_count", C.POINTER(C.c_int32)), ("ring_len", C.POINTER(C.c_int32)),
                ("xy", C.POINTER(C.c_int16)), ("poly_cap", C.c_uint64), ("ring_cap", C.c_uint64), ("vertex_cap", C.c_uint64),
                ("n_polygons", C.c_uint64), ("n_rings", C.c_uint64), ("n_vertices", C.c_uint64), ("n_flagged", C.c_uint64),
                ("crops", C.POINTER(RsMaskCrops)), ("want_masks", C.c_int32), ("masks_copied", C.c_int32)]


POLY_HDR = 8       # RS_POLY_HDR: flagged, polygons, rings, vertices, first polygon, first ring, first vertex, 0


class RsEvalCounts(C.Structure):
    _fields_ = [("inter", C.POINTER(C.c_int32)), ("det_area", C.POINTER(C.c_int32)), ("gt_area", C.POINTER(C.c_int32))]


class RsEvalMatches(C.Structure):
    _fields_ = [("order", C.POINTER(C.c_int32)), ("class_first", C.POINTER(C.c_int32)), ("gt_per_class", C.POINTER(C.c_int32)),
                ("matched", C.POINTER(C.c_uint32)), ("ignored", C.POINTER(C.c_uint32)), ("npig", C.POINTER(C.c_int32))]


class RsRoadVotes(C.Structure):
    _fields_ = [("wscore", C.POINTER(C.c_double)), ("wfrac", C.POINTER(C.c_double)), ("pairs", C.POINTER(C.c_int32)),
                ("label_area", C.POINTER(C.c_int32))]


class RsRoadVotesPoly(C.Structure):
    """include/rs_engine.h ``rs_road_votes_poly``: the sweep's tables on polygon areas, float64 label areas and the flagged counts."""
    _fields_ = [("wscore", C.POINTER(C.c_double)), ("wfrac", C.POINTER(C.c_double)), ("pairs", C.POINTER(C.c_int32)),
                ("label_area", C.POINTER(C.c_double)), ("flagged", C.POINTER(C.c_int32))]


class RsRoadVoteSweep(C.Structure):
    """include/rs_engine.h ``rs_road_vote_sweep``: the tables of ``RsRoadVotes`` with a threshold axis behind the tile's."""
    _fields_ = [("wscore", C.POINTER(C.c_double)), ("wfrac", C.POINTER(C.c_double)), ("pairs", C.POINTER(C.c_int32)),
                ("label_area", C.POINTER(C.c_int32))]


class RsBandHist(C.Structure):
    _fields_ = [("hist", C.POINTER(C.c_uint32))]


class RsSolver(C.Structure):
    """include/rs_engine.h ``rs_solver``."""
    _fields_ = [("struct_size", C.c_int32), ("nesterov", C.c_int32), ("bias_lr_factor", C.c_float), ("weight_decay_bias", C.c_float),
                ("has_weight_decay_bias", C.c_int32), ("clip_type", C.c_int32), ("clip_value", C.c_float), ("norm_type", C.c_float)]


CLIP_TYPES = ("none", "value", "norm", "full_model")     # rs_solver.clip_type 0..3


class SolverOptions:
    """The optimiser step's options beyond lr / momentum / weight decay, under detectron2's SOLVER keys: ``nesterov`` (NESTEROV),
    ``bias_lr_factor`` (BIAS_LR_FACTOR), ``weight_decay_bias`` (WEIGHT_DECAY_BIAS; ``None`` = biases decay as the weights do),
    ``clip_type`` (CLIP_GRADIENTS: "none" = ENABLED false, "value" / "norm" per parameter tensor as detectron2 0.6 clips, "full_model" =
    one norm over all of them, the extension of detectron2's DETR / Mask2Former projects), ``clip_value`` (CLIP_VALUE), ``norm_type``
    (NORM_TYPE: 2.0 or ``float("inf")``).  The defaults are torch.optim.SGD as the trainer always ran it.  WEIGHT_DECAY_NORM has no
    field: every norm layer of this model is a FrozenBN."""

    def __init__(self, nesterov: bool = False, bias_lr_factor: float = 1.0, weight_decay_bias: Optional[float] = None,
                 clip_type: str = "none", clip_value: float = 1.0, norm_type: float = 2.0):
        if clip_type not in CLIP_TYPES:
            raise ValueError(f"clip_type must be one of {CLIP_TYPES}, got {clip_type!r}")
        self.nesterov, self.bias_lr_factor, self.weight_decay_bias = bool(nesterov), float(bias_lr_factor), weight_decay_bias
        self.clip_type, self.clip_value, self.norm_type = clip_type, float(clip_value), float(norm_type)

    def to_struct(self) -> RsSolver:
        wdb = self.weight_decay_bias
        return RsSolver(C.sizeof(RsSolver), int(self.nesterov), self.bias_lr_factor, 0.0 if wdb is None else float(wdb), 0 if wdb is None else 1,
                        CLIP_TYPES.index(self.clip_type), self.clip_value, self.norm_type)

    def __repr__(self) -> str:
        return (f"SolverOptions(nesterov={self.nesterov}, bias_lr_factor={self.bias_lr_factor}, weight_decay_bias={self.weight_decay_bias}, "
                f"clip_type={self.clip_type!r}, clip_value={self.clip_value}, norm_type={self.norm_type})")


class PolygonTables:
    """Polygons of the instances of one tile as the device polygoniser leaves them (include/rs_engine.h, ``rs_op_polygonize``):
    ``header`` (n, 8) int32 per instance [flagged, polygons, rings, vertices, first polygon, first ring, first vertex, 0] with the
    offsets pointing into ``poly_ring_count`` / ``ring_len`` / ``xy`` ((nv, 2) int16, tile pixels); ``rdp_epsilon`` is the tolerance
    they were simplified with (0.0 = not simplified).  A flagged instance has no rows here: its mask exceeded the kernel's
    capacities and is vectorised on the host from its crop (``proj_roadsurf_amd.vectorize``)."""

    def __init__(self, header: np.ndarray, poly_ring_count: np.ndarray, ring_len: np.ndarray, xy: np.ndarray, rdp_epsilon: float,
                 totals: Optional[np.ndarray] = None):
        self.header = np.ascontiguousarray(header, np.int32).reshape(-1, POLY_HDR)
        self.poly_ring_count = np.ascontiguousarray(poly_ring_count, np.int32)
        self.ring_len = np.ascontiguousarray(ring_len, np.int32)
        self.xy = np.ascontiguousarray(xy, np.int16).reshape(-1, 2)
        self.rdp_epsilon = max(float(rdp_epsilon), 0.0)
        # the stand-alone operator's totals [polygons, rings, vertices, flagged instances] as the device summed them (None: not carried)
        self.totals = None if totals is None else np.asarray(totals, np.int32).copy()

    @property
    def flagged(self) -> np.ndarray:
        return np.nonzero(self.header[:, 0])[0]


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load librs_engine.so (built in-tree by ``__graft_entry__.build()`` / csrc/Makefile)."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    try:
        # PyTorch-ROCm wheels bundle their own libamdhip64; librs_engine.so links the system one (/opt/rocm).  If ours is loaded
        # first and torch later initialises the GPU through its copy, the second HIP runtime of the process reports "no
        # ROCm-capable device".  Importing torch first (when it is installed -- tests, bench.py and the data-parallel trainer use it)
        # lets both bind to ONE runtime; the engine itself never calls into torch.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise RsError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc, gfx950). There is no CPU fallback for the detection path.")
    lib = C.CDLL(p)
    vp, i32, f32p, i32p, u8p = C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    lib.rs_last_error.restype = C.c_char_p
    lib.rs_abi_version.restype = i32
    lib.rs_engine_create.argtypes = [C.POINTER(RsSpec), vp, C.c_size_t, i32, i32, i32, i32, i32, vp, C.POINTER(vp)]
    lib.rs_engine_destroy.argtypes = [vp]
    lib.rs_engine_destroy.restype = None
    lib.rs_engine_infer.argtypes = [vp, vp, i32, C.POINTER(RsDets)]
    lib.rs_engine_infer_device.argtypes = [vp, vp, i32]
    lib.rs_engine_infer_phase.argtypes = [vp, vp, i32, i32]
    lib.rs_engine_sync.argtypes = [vp]
    lib.rs_host_alloc.argtypes = [C.c_size_t]
    lib.rs_host_alloc.restype = vp
    lib.rs_host_free.argtypes = [vp]
    lib.rs_host_free.restype = None
    lib.rs_engine_upload_async.argtypes = [vp, vp, i32]
    lib.rs_engine_fetch_async.argtypes = [vp, i32, C.POINTER(RsDets)]
    lib.rs_engine_fetch_wait.argtypes = [vp]
    lib.rs_engine_fetch_crops_async.argtypes = [vp, i32, C.POINTER(RsDets), C.POINTER(RsMaskCrops)]
    lib.rs_engine_fetch_crops_wait.argtypes = [vp, C.POINTER(RsMaskCrops)]
    lib.rs_engine_fetch_polygons_async.argtypes = [vp, i32, C.POINTER(RsDets), C.POINTER(RsPolygons), C.c_double]
    lib.rs_engine_fetch_polygons_wait.argtypes = [vp, C.POINTER(RsPolygons)]
    lib.rs_engine_fetch.argtypes = [vp, i32, C.POINTER(RsDets)]
    lib.rs_engine_stream.argtypes = [vp]
    lib.rs_engine_stream.restype = vp
    lib.rs_engine_set_profiling.argtypes = [vp, i32]
    lib.rs_debug_run_stages_matching.argtypes = [vp, C.c_char_p, i32]
    lib.rs_engine_stage_count.argtypes = [vp]
    lib.rs_engine_saturation.argtypes = [vp, C.POINTER(C.c_int64), i32]
    lib.rs_op_set_saturation_counter.argtypes = [vp]
    lib.rs_engine_stage_info.argtypes = [vp, i32, C.c_char_p, C.POINTER(C.c_double), i32p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.rs_engine_stage_kernel.argtypes = [vp, i32, C.c_char_p]
    lib.rs_engine_stage_variant.argtypes = [vp, i32]
    lib.rs_op_conv_variant.argtypes = [i32] * 7 + [i32p]
    if hasattr(lib, "rs_op_conv_variant_split"):      # RS_ENGINE_LIB may name an older build (A/B measurements against a parent commit)
        lib.rs_op_conv_variant_split.argtypes = [i32] * 7 + [i32p]
    lib.rs_engine_tensor.argtypes = [vp, C.c_char_p, C.POINTER(vp), i32p, i32p, C.POINTER(C.c_int64), i32p]
    lib.rs_engine_tensor_count.argtypes = [vp]
    lib.rs_engine_tensor_name.argtypes = [vp, i32, C.c_char_p]
    lib.rs_engine_net_shape.argtypes = [vp, i32p, i32p, i32p, i32p]
    lib.rs_op_conv2d.argtypes = [vp, vp, vp, vp, vp, vp] + [i32] * 17 + [vp]
    lib.rs_op_bneck_tail.argtypes = [vp] * 12 + [i32, i32, i32, i32, vp]
    lib.rs_op_conv2d_dual.argtypes = [vp, vp, vp, vp, vp] + [i32] * 19 + [vp]
    i64 = C.c_int64
    lib.rs_op_conv2d_split.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, i64] + [i32] * 16 + [vp]
    lib.rs_op_bneck_tail_split.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, vp]
    if hasattr(lib, "rs_op_deconv_predict_split"):
        lib.rs_op_deconv_predict_split.argtypes = [vp, i64, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.rs_op_conv2d_dgrad.argtypes = [vp] * 7 + [i32] * 14 + [vp]
    lib.rs_op_conv2d_wgrad.argtypes = [vp, vp, vp, vp] + [i32] * 13 + [vp]
    lib.rs_op_conv2d_wgrad_split.argtypes = lib.rs_op_conv2d_wgrad.argtypes
    lib.rs_op_conv2d_wgrad_split_serves.argtypes = [i32, i32]
    if hasattr(lib, "rs_op_stem_wgrad"):              # RS_ENGINE_LIB may name an older build
        lib.rs_op_maxpool3x3s2_bwd.argtypes = [vp, vp, vp] + [i32] * 7 + [vp]
        lib.rs_op_stem_wgrad.argtypes = [vp, vp, vp, vp] + [i32] * 7 + [vp]
        lib.rs_op_stem_wgrad_f32.argtypes = lib.rs_op_stem_wgrad.argtypes
    if hasattr(lib, "rs_op_conv2d_dgrad_split"):      # RS_ENGINE_LIB may name an older build
        lib.rs_op_conv2d_dgrad_split.argtypes = [vp] * 7 + [i32] * 14 + [vp, vp]
        lib.rs_op_conv2d_dgrad_split_serves.argtypes = [i32, i32, i32, i32]
    if hasattr(lib, "rs_op_conv2d_fwd_split"):
        lib.rs_op_conv2d_fwd_split.argtypes = [vp] * 6 + [i32] * 14 + [vp, vp]
        lib.rs_op_conv2d_fwd_split_serves.argtypes = [i32, i32, i32, i32]
        lib.rs_op_split_rows.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.rs_op_nms.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp]
    lib.rs_op_batched_nms.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, i32, vp]
    lib.rs_op_batched_nms_decision.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, i32, vp, vp, vp]
    lib.rs_op_det_merge.argtypes = [vp] * 5 + [i32] * 4 + [C.c_float] * 4 + [vp] * 7
    lib.rs_spec_batched_nms.argtypes = [C.POINTER(RsSpec)]
    lib.rs_op_roi_align.argtypes = [C.POINTER(vp), i32p, i32p, f32p, i32, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.rs_op_roi_align_bwd.argtypes = [C.POINTER(vp), i32p, i32p, f32p, i32, vp, i32, i32, i32, i32, vp, vp]
    if hasattr(lib, "rs_op_roi_align_form"):          # RS_ENGINE_LIB may name an older build
        lib.rs_op_roi_align_form.argtypes = [C.POINTER(vp), C.POINTER(i64), i32p, i32p, f32p, i32, vp, i32, i32, i32, i32, i32, vp, i64] + [vp] * 6
        lib.rs_op_roi_align_bwd_form.argtypes = [C.POINTER(vp), i32p, i32p, f32p, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    f32 = C.c_float
    lib.rs_op_match.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, i32, i32, i32, vp]
    lib.rs_op_subsample.argtypes = [vp, vp, vp, i32, i32, i32, f32, i32, i32, C.c_uint32, vp]
    lib.rs_op_rpn_loss.argtypes = [vp] * 6 + [i32] * 6 + [f32, f32, vp]
    lib.rs_op_box_loss.argtypes = [vp] * 6 + [i32, i32, i32, f32, f32p, f32, vp]
    lib.rs_op_mask_loss.argtypes = [vp] * 5 + [i32, i32, i32, f32, vp]
    lib.rs_op_sgd_momentum.argtypes = [vp, vp, vp, C.c_int64, f32, f32, f32, f32, i32, vp]
    lib.rs_op_fold_weights.argtypes = [vp] * 4 + [i32] * 6 + [vp]
    if hasattr(lib, "rs_op_label_counts"):            # RS_ENGINE_LIB may name an older build
        lib.rs_op_label_counts.argtypes = [vp, C.c_int64, vp, vp]
        lib.rs_op_box_stats.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp, vp]
        lib.rs_op_mask_stats.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
        lib.rs_host_label_counts.argtypes = [vp, C.c_int64, vp]
        lib.rs_host_box_stats.argtypes = [vp, vp, i32, i32, i32, vp, i32, vp]
        lib.rs_host_mask_stats.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
        lib.rs_trainer_set_train_stats.argtypes = [vp, i32]
    if hasattr(lib, "rs_op_sgd_segments"):            # RS_ENGINE_LIB may name an older build
        lib.rs_op_sgd_segments.argtypes = [vp, vp, vp, i64, vp, vp, vp, i32, f32, f32, f32, f32, C.POINTER(RsSolver), vp, vp, vp, vp]
        lib.rs_host_sgd_segments.argtypes = [vp, vp, vp, i64, vp, vp, vp, i32, f32, f32, f32, f32, C.POINTER(RsSolver), vp, vp, vp]
        lib.rs_trainer_set_solver.argtypes = [vp, C.POINTER(RsSolver)]
        lib.rs_trainer_segment_count.argtypes = [vp]
        lib.rs_trainer_segment_info.argtypes = [vp, i32, C.c_char_p, C.POINTER(i64), C.POINTER(i64), i32p]
    lib.rs_resize_shape.argtypes = [i32, i32, i32, i32, i32p, i32p]
    lib.rs_resize_shape.restype = None
    lib.rs_resize_coeffs.argtypes = [i32, i32, i32p, i32p]
    i64p, f64p = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    lib.rs_vectorize_masks.argtypes = [vp, i32, i32, i32, C.c_double, i32]
    lib.rs_vectorize_masks.restype = vp
    lib.rs_vec_counts.argtypes = [vp, i64p, i64p, i64p, i64p]
    lib.rs_vec_counts.restype = None
    lib.rs_vec_copy.argtypes = [vp, i32p, i32p, i32p, f64p]
    lib.rs_vec_free.argtypes = [vp]
    lib.rs_vec_free.restype = None
    lib.rs_vectorize_mask_crops.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, i32]
    lib.rs_vectorize_mask_crops.restype = vp
    lib.rs_vec_from_tables.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.rs_vec_from_tables.restype = vp
    lib.rs_polygonize_caps.argtypes = [i32p, i32p, i32p, i32p]
    lib.rs_polygonize_caps.restype = None
    lib.rs_op_polygonize.argtypes = [vp, i32, i32, i32, C.c_double, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.rs_op_polygonize_crops.argtypes = [vp, i32, i32, vp, vp, i32, i32, C.c_double, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.rs_op_rasterize_canvas.argtypes = [vp] * 4 + [i32, i32, vp]
    lib.rs_op_mask_pair_counts.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.rs_engine_eval_fits.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.rs_engine_fetch_eval_async.argtypes = [vp, i32, C.POINTER(RsDets), vp, vp, vp, vp, vp, C.POINTER(RsEvalCounts)]
    lib.rs_engine_fetch_eval_wait.argtypes = [vp]
    if hasattr(lib, "rs_op_coco_match"):              # RS_ENGINE_LIB may name an older build
        lib.rs_op_coco_match.argtypes = [vp] * 11 + [i32] * 4 + [vp] * 7
        lib.rs_host_coco_match.argtypes = [vp] * 11 + [i32] * 4 + [vp] * 6
        lib.rs_engine_fetch_eval_match_async.argtypes = [vp, i32, C.POINTER(RsDets)] + [vp] * 8 + [C.POINTER(RsEvalMatches)]
        lib.rs_engine_fetch_eval_match_wait.argtypes = [vp]
    if hasattr(lib, "rs_op_road_votes"):              # RS_ENGINE_LIB may name an older build
        lib.rs_op_road_votes.argtypes = [vp] * 6 + [i32] * 4 + [C.c_double] + [vp] * 4
        lib.rs_host_road_votes.argtypes = [vp] * 6 + [i32] * 4 + [C.c_double] + [vp] * 3
        lib.rs_engine_fetch_votes_async.argtypes = [vp, i32] + [vp] * 5 + [C.c_double, C.POINTER(RsRoadVotes)]
        lib.rs_engine_fetch_votes_wait.argtypes = [vp]
    if hasattr(lib, "rs_op_road_votes_sweep"):        # RS_ENGINE_LIB may name an older build
        lib.rs_op_road_votes_sweep.argtypes = [vp] * 6 + [i32] * 4 + [vp, i32] + [vp] * 4
        lib.rs_host_road_votes_sweep.argtypes = [vp] * 6 + [i32] * 4 + [vp, i32] + [vp] * 3
        lib.rs_engine_fetch_vote_sweep_async.argtypes = [vp, i32] + [vp] * 5 + [vp, i32, C.POINTER(RsRoadVoteSweep)]
        lib.rs_engine_fetch_vote_sweep_wait.argtypes = [vp]
    if hasattr(lib, "rs_engine_fetch_votes_poly_async"):   # RS_ENGINE_LIB may name an older build
        lib.rs_engine_fetch_votes_poly_async.argtypes = [vp, i32] + [vp] * 5 + [vp, i32, C.POINTER(RsRoadVotesPoly)]
        lib.rs_engine_fetch_votes_poly_wait.argtypes = [vp]
    if hasattr(lib, "rs_op_band_hist"):              # RS_ENGINE_LIB may name an older build
        lib.rs_op_band_hist.argtypes = [vp] * 3 + [i32] * 4 + [vp, vp]
        lib.rs_host_band_hist.argtypes = [vp] * 3 + [i32] * 4 + [vp]
        lib.rs_engine_fetch_band_hist_async.argtypes = [vp, i32] + [vp] * 5 + [C.POINTER(RsBandHist)]
        lib.rs_engine_fetch_band_hist_wait.argtypes = [vp]
    lib.rs_rasterize_polygons_within_box.argtypes = [f64p, i32p, i32, f64p, i32, u8p]
    lib.rs_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
    lib.rs_op_fdiv.argtypes = [vp, vp, vp, C.c_int64, vp]
    lib.rs_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
    if path is None:
        _LIB = lib
    return lib


def _check(lib: C.CDLL, rc: int, what: str) -> None:
    if rc != 0:
        raise RsError(f"{what} failed ({rc}): {lib.rs_last_error().decode(errors='replace')}")


def cell_anchor_table(spec: EngineSpec) -> np.ndarray:
    """``DefaultAnchorGenerator.generate_cell_anchors`` [EXT d2: modeling/anchor_generator.py]
    (R:45-56): float64 arithmetic, stored as fp32.  Shape (levels, anchors, 4)."""
    out = np.zeros((len(spec.anchor_sizes), spec.num_anchors, 4), np.float32)
    for l, sizes in enumerate(spec.anchor_sizes):
        a = 0
        for size in sizes:
            area = float(size) ** 2.0
            for ar in spec.anchor_aspect_ratios:
                w = math.sqrt(area / ar)
                h = ar * w
                out[l, a] = (-w / 2.0, -h / 2.0, w / 2.0, h / 2.0)
                a += 1
    return out


def nms_thresh_f32(t: float) -> float:
    """The largest float32 <= t.  torchvision's nms compares the fp32 IoU with its threshold as a C++ double
    (``ovr > iou_threshold``); the kernels compare in fp32 (include/rs_engine.h, rs_op_nms), and for a float IoU x,
    x > t exactly when x > nms_thresh_f32(t).  Rounding t to nearest instead would keep a pair whose IoU is
    float32(t) whenever float32(t) > t (0.3, 0.4, 0.6, ...)."""
    f = np.float32(t)
    if float(f) > t:
        f = np.nextafter(f, np.float32(-np.inf))
    return float(f)


def make_rs_spec(spec: EngineSpec) -> RsSpec:
    spec.check_supported()
    s = RsSpec()
    s.struct_size = C.sizeof(RsSpec)
    s.in_channels = spec.in_channels
    s.flip_channels = 1 if spec.input_format == "RGB" else 0
    for i in range(spec.in_channels):
        s.pixel_mean[i] = spec.pixel_mean[i]
        s.pixel_std[i] = spec.pixel_std[i]
    s.min_size_test, s.max_size_test, s.size_divisibility = spec.min_size_test, spec.max_size_test, spec.size_divisibility
    for i, b in enumerate(spec.res_blocks):
        s.res_blocks[i] = b
    s.stem_out_channels, s.res2_out_channels = spec.stem_out_channels, spec.res2_out_channels
    s.stride_in_1x1 = int(spec.stride_in_1x1)
    s.fpn_out_channels = spec.fpn_out_channels
    s.num_levels, s.num_anchors = len(spec.rpn_in_features), spec.num_anchors
    if s.num_levels > MAX_LEVELS or s.num_anchors > MAX_ANCHORS:
        raise RsError("too many RPN levels / anchors")
    ca = cell_anchor_table(spec)
    for l in range(ca.shape[0]):
        for a in range(ca.shape[1]):
            for d in range(4):
                s.cell_anchors[l][a][d] = float(ca[l, a, d])
    s.anchor_offset = spec.anchor_offset
    for i in range(4):
        s.rpn_bbox_reg_weights[i] = spec.rpn_bbox_reg_weights[i]
        s.box_reg_weights[i] = spec.box_reg_weights[i]
    s.rpn_pre_nms_topk, s.rpn_post_nms_topk = spec.rpn_pre_nms_topk_test, spec.rpn_post_nms_topk_test
    s.rpn_nms_thresh, s.rpn_min_size = nms_thresh_f32(spec.rpn_nms_thresh), spec.rpn_min_size
    s.num_classes = spec.num_classes
    s.score_thresh_test, s.nms_thresh_test = spec.score_thresh_test, nms_thresh_f32(spec.nms_thresh_test)
    s.detections_per_image = spec.detections_per_image
    s.box_fc_dim, s.box_pooler_resolution = spec.box_fc_dim, spec.box_pooler_resolution
    s.mask_on, s.mask_pooler_resolution = int(spec.mask_on), spec.mask_pooler_resolution
    s.mask_num_conv, s.mask_conv_dim = spec.mask_num_conv, spec.mask_conv_dim
    s.mask_threshold, s.scale_clamp = spec.mask_threshold, spec.scale_clamp
    s.precision = {"fp16": 0, "fp32": 1, "split": 2}[spec.precision]
    s.batched_nms = BATCHED_NMS_MODES.index(spec.batched_nms)
    return s


class Instances:
    """Numpy-backed stand-in for detectron2 ``Instances`` ([EXT d2: structures/instances.py]) with the
    four fields the object-detector reads: ``pred_boxes`` (n,4 XYXY abs, tile pixels), ``scores``,
    ``pred_classes``, ``pred_masks`` (n,H,W bool).  Sorted by score, descending."""

    def __init__(self, image_size: Tuple[int, int], pred_boxes: np.ndarray, scores: np.ndarray, pred_classes: np.ndarray,
                 packed_masks: Optional[np.ndarray], mask_probs: Optional[np.ndarray],
                 crops: Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]] = None, polygons: Optional[PolygonTables] = None):
        self.image_size = image_size
        self.pred_boxes = pred_boxes
        self.scores = scores
        self.pred_classes = pred_classes
        self._packed_full = packed_masks
        self.mask_probs = mask_probs
        # masks as crops of their boxes (rs_mask_crops): (rects (n,4) int32 [first byte column, first row, bytes per row, rows],
        # offsets (n,) uint32 into data, data uint8); the full canvases are rebuilt on demand
        self._crops = crops
        # polygons traced on the device (Engine.fetch_async(polygons=True)) with the epsilon they were simplified with; masks come
        # along only when the caller asked for them or an instance of the batch was left to the host vectoriser
        self._polygons = polygons

    @property
    def _packed(self) -> Optional[np.ndarray]:
        """Bit-packed full-canvas masks (n, h, ceil(w/8)); rebuilt from the crops when the masks arrived cropped."""
        if self._packed_full is None and self._crops is not None:
            h, w = self.image_size
            rects, offs, data = self._crops
            full = np.zeros((len(self), h, (w + 7) // 8), np.uint8)
            for i in range(len(self)):
                x0b, y0, wb, rows = (int(v) for v in rects[i])
                if wb > 0 and rows > 0:
                    o = int(offs[i])
                    full[i, y0:y0 + rows, x0b:x0b + wb] = data[o:o + wb * rows].reshape(rows, wb)
            self._packed_full = full
        return self._packed_full

    def __len__(self) -> int:
        return int(self.scores.shape[0])

    def has(self, name: str) -> bool:
        return name in ("pred_boxes", "scores", "pred_classes") or (name == "pred_masks" and (self._packed_full is not None or self._crops is not None))

    @property
    def pred_masks(self) -> np.ndarray:
        if self._packed is None:
            raise AttributeError("pred_masks not computed (MASK_ON false)")
        h, w = self.image_size
        if len(self) == 0:
            return np.zeros((0, h, w), bool)
        bits = np.unpackbits(self._packed, axis=-1, bitorder="little")[:, :, :w]
        return bits.astype(bool)

    def to(self, *_a: Any, **_k: Any) -> "Instances":   # ``instances.to("cpu")`` in caller code
        return self

    def get_fields(self) -> Dict[str, Any]:
        d = {"pred_boxes": self.pred_boxes, "scores": self.scores, "pred_classes": self.pred_classes}
        if self.has("pred_masks"):
            d["pred_masks"] = self.pred_masks
        return d


_REGISTERED_HOST: List[Tuple[int, int, Any]] = []        # ([lo, hi) address range pinned with rs_host_register, weak reference to the array)


def _registered_view(a: np.ndarray) -> bool:
    """Is ``a`` (a view of) an array pinned by ``register_host_buffer``?  Address AND object identity: an unrelated array that
    happens to sit at the address of a slab that has gone away must not pass for pinned."""
    if not a.flags.c_contiguous:
        return False
    addr = a.ctypes.data
    for lo, hi, buf in _REGISTERED_HOST:
        if lo <= addr and addr + a.nbytes <= hi and buf() is not None and (a is buf() or a.base is buf()):
            return True
    return False


def register_host_buffer(buf: np.ndarray, lib_path: Optional[str] = None) -> bool:
    """Pin the memory behind ``buf`` (e.g. ``decode_pool.DecodePool.slab``, a shared-memory array that decoder processes fill) so
    that ``Engine.upload_async`` / ``LanePipeline.run`` copy batches that are views of it straight to the device instead of
    staging them through the engine's own pinned buffer (a 12.6 MB memcpy per batch of 16 512x512 tiles on the thread that feeds
    the GPU).  The caller must leave a batch untouched until the forward that consumed it has delivered its results.  Returns
    False (and changes nothing) if the runtime refuses to pin the range."""
    lib = load_library(lib_path)
    lib.rs_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lo = buf.ctypes.data
    if lib.rs_host_register(C.c_void_p(lo), buf.nbytes) != 0:
        return False
    _REGISTERED_HOST.append((lo, lo + buf.nbytes, weakref.ref(buf)))
    return True


def unregister_host_buffer(buf: np.ndarray, lib_path: Optional[str] = None) -> None:
    lib = load_library(lib_path)
    lib.rs_host_unregister.argtypes = [C.c_void_p]
    lo = buf.ctypes.data
    for r in list(_REGISTERED_HOST):
        if r[0] == lo:
            _REGISTERED_HOST.remove(r)
            lib.rs_host_unregister(C.c_void_p(lo))


class Engine:
    """One engine = one process, one GPU, one tile shape, batches up to ``max_batch``."""

    def __init__(self, spec: EngineSpec, weights: Dict[str, np.ndarray], tile_shape: Tuple[int, int, int], max_batch: int = 16,
                 device: int = 0, stream: Optional[int] = None, lib_path: Optional[str] = None, blob: Optional[bytes] = None):
        """``blob``: the result of ``pack_weights(spec, weights)`` when the caller already has it (LanePipeline packs once for all lanes)."""
        self.lib = load_library(lib_path)
        if self.lib.rs_abi_version() != 1:
            raise RsError("librs_engine.so ABI version mismatch")
        self.spec = spec
        self.tile_h, self.tile_w, self.tile_c = (int(x) for x in tile_shape)
        self.max_batch = int(max_batch)
        self.D = spec.detections_per_image
        if blob is None:
            blob = pack_weights(spec, weights)
        rs = make_rs_spec(spec)
        h = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        rc = self.lib.rs_engine_create(C.byref(rs), buf, len(blob), device, self.max_batch, self.tile_h, self.tile_w, self.tile_c,
                                       C.c_void_p(stream) if stream else None, C.byref(h))
        _check(self.lib, rc, "rs_engine_create")
        self._h = h
        self._alloc_out(self.max_batch)

    @classmethod
    def from_handle(cls, lib: C.CDLL, handle: int, spec: EngineSpec, tile_shape: Tuple[int, int, int], max_batch: int) -> "Engine":
        """Wrap an engine owned by someone else (the trainer's forward engine: ``rs_trainer_engine``) for inference calls;
        ``close`` frees only this wrapper's pinned host buffers."""
        self = cls.__new__(cls)
        self.lib, self.spec = lib, spec
        self.tile_h, self.tile_w, self.tile_c = (int(x) for x in tile_shape)
        self.max_batch, self.D = int(max_batch), spec.detections_per_image
        self._h = C.c_void_p(handle)
        self._borrowed = True
        self._alloc_out(self.max_batch)
        return self

    # ------------------------------------------------------------------ plumbing
    def _pinned(self, shape: Tuple[int, ...], dtype) -> np.ndarray:
        """numpy array over pinned host memory (rs_host_alloc): device<->host copies run at PCIe speed and asynchronously."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.lib.rs_host_alloc(max(nbytes, 16))
        if not ptr:
            raise RsError(f"rs_host_alloc({nbytes}) failed")
        self._pinned_ptrs.append(ptr)
        a = np.ctypeslib.as_array((C.c_uint8 * max(nbytes, 1)).from_address(ptr))[:nbytes].view(dtype).reshape(shape)
        a[...] = 0
        return a

    def _alloc_out(self, n: int) -> None:
        D, h, wb = self.D, self.tile_h, (self.tile_w + 7) // 8
        self._pinned_ptrs: List[int] = []
        self._count = self._pinned((n,), np.int32)
        self._boxes = self._pinned((n, D, 4), np.float32)
        self._scores = self._pinned((n, D), np.float32)
        self._classes = self._pinned((n, D), np.int32)
        self._masks = self._pinned((n, D, h, wb), np.uint8) if self.spec.mask_on else None
        self._probs = np.zeros((n, D, MASK_SIDE, MASK_SIDE), np.float32) if self.spec.mask_on else None
        self._stage_tiles = self._pinned((n, self.tile_h, self.tile_w, self.tile_c), np.uint8)
        # masks as crops (rs_engine_fetch_crops_*): table + data; the data buffer is pinned lazily on first use
        self._crop_rects = self._pinned((n, D, 4), np.int32) if self.spec.mask_on else None
        self._crop_offsets = self._pinned((n, D), np.uint32) if self.spec.mask_on else None
        self._crop_data: Optional[np.ndarray] = None
        self._crops_struct: Optional[RsMaskCrops] = None
        # polygons (rs_engine_fetch_polygons_*): pinned tables, allocated on the first polygon fetch
        self._poly_struct: Optional[RsPolygons] = None
        self._poly_eps = 0.0
        # the kind of fetch_async that is in flight, and of the one wait_results waited for last: None, "canvas", "crops" or "polygons"
        self._fetch_pending: Optional[str] = None
        self._fetch_landed: Optional[str] = None
        # validation counts (rs_engine_fetch_eval_*): pinned tables, allocated on the first eval_counts; batches that did not fit
        self._eval_struct: Optional[RsEvalCounts] = None
        self._match_struct: Optional[RsEvalMatches] = None
        self.eval_fallbacks = 0
        self.eval_unpack_s = 0.0             # eval_matches: seconds spent turning the tables into records (tools/val_ap_ab.py reads it)
        # road votes (rs_engine_fetch_votes_*): pinned tables, allocated on the first road_votes; batches that did not fit
        self._vote_struct: Optional[RsRoadVotes] = None
        self._vote_labels: List[int] = []
        # the vote sweep (rs_engine_fetch_vote_sweep_*): pinned tables for 32 thresholds, allocated on the first road_votes_sweep
        self._sweep_struct: Optional[RsRoadVoteSweep] = None
        self._sweep_labels: Tuple[List[int], int] = ([], 0)
        # the polygon geometry of the vote (rs_engine_fetch_votes_poly_*): pinned tables, allocated on the first call that asks for it
        self._pvote_struct: Optional[RsRoadVotesPoly] = None
        self._pvote_labels: Tuple[List[int], int] = ([], 0)
        self._pvote_batch = None                     # (labels, thresholds) of the batch in flight, for the host route of a flagged tile
        self.vote_fallbacks = 0
        # band histograms (rs_engine_fetch_band_hist_*): one pinned table, allocated on the first band_hist; batches that did not fit
        self._band_struct: Optional[RsBandHist] = None
        self._band_labels: List[int] = []
        self._band_pending = False           # a band_hist fetch the host has not waited for: the device may still be reading the tiles
        self.band_fallbacks = 0

    def _dets_struct(self, want_probs: bool) -> RsDets:
        d = RsDets()
        d.count = self._count.ctypes.data_as(C.POINTER(C.c_int32))
        d.boxes = self._boxes.ctypes.data_as(C.POINTER(C.c_float))
        d.scores = self._scores.ctypes.data_as(C.POINTER(C.c_float))
        d.classes = self._classes.ctypes.data_as(C.POINTER(C.c_int32))
        if self._masks is not None:
            d.masks = self._masks.ctypes.data_as(C.POINTER(C.c_uint8))
            if want_probs:
                d.mask_probs = self._probs.ctypes.data_as(C.POINTER(C.c_float))
        return d

    # The mask payload of tile i (c detections) as Instances takes it, one function per kind of fetch
    def _tile_canvas(self, i: int, c: int, want_probs: bool = False) -> Dict[str, Any]:
        return dict(packed_masks=self._masks[i, :c].copy() if self._masks is not None else None,
                    mask_probs=self._probs[i, :c].copy() if (self._probs is not None and want_probs) else None)

    def _tile_crops(self, i: int, c: int, want_probs: bool = False) -> Dict[str, Any]:
        rects = self._crop_rects[i, :c].copy()
        offs = self._crop_offsets[i, :c].astype(np.int64)
        if c:
            lo = int(offs[0])
            hi = int(offs[c - 1]) + int(rects[c - 1, 2]) * int(rects[c - 1, 3])
            data = self._crop_data[lo:hi].copy()          # the tile's crops are contiguous, in slot order
            offs = (offs - lo).astype(np.uint32)
        else:
            data, offs = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        return dict(packed_masks=None, mask_probs=None, crops=(rects, offs, data))

    def _tile_polygons(self, i: int, c: int, want_probs: bool = False) -> Dict[str, Any]:
        hdr = self._poly_header[i, :c].copy()
        if c:
            lo = hdr[0, 4:7].copy()
            hi = hdr[c - 1, 4:7] + hdr[c - 1, 1:4]
            hdr[:, 4:7] -= lo
        else:
            lo = hi = np.zeros(3, np.int32)
        tables = PolygonTables(hdr, self._poly_prc[lo[0]:hi[0]].copy(), self._poly_rlen[lo[1]:hi[1]].copy(),
                               self._poly_xy[lo[2]:hi[2]].copy(), self._poly_eps)
        masks = self._tile_crops(i, c) if self._poly_struct.masks_copied else dict(packed_masks=None, mask_probs=None)
        return dict(masks, polygons=tables)

    def _collect(self, n: int, want_probs: bool, kind: str = "canvas") -> List[Instances]:
        """``Instances`` of tiles 0..n-1 out of the pinned buffers; ``kind``: what the fetch left there for the masks."""
        masks_of = {"canvas": self._tile_canvas, "crops": self._tile_crops, "polygons": self._tile_polygons}[kind]
        out = []
        for i in range(n):
            c = int(self._count[i])
            out.append(Instances((self.tile_h, self.tile_w), self._boxes[i, :c].copy(), self._scores[i, :c].copy(),
                                 self._classes[i, :c].astype(np.int64), **masks_of(i, c, want_probs)))
        return out

    # ------------------------------------------------------------------ inference
    def infer(self, tiles: np.ndarray, want_probs: bool = False) -> List[Instances]:
        """tiles: (n, h, w, c) uint8, BGR as ``cv2.imread`` returns them.  Returns one ``Instances`` per tile."""
        tiles = np.ascontiguousarray(tiles)
        if tiles.dtype != np.uint8 or tiles.ndim != 4 or tiles.shape[1:] != (self.tile_h, self.tile_w, self.tile_c):
            raise ValueError(f"tiles must be uint8 (n,{self.tile_h},{self.tile_w},{self.tile_c}), got {tiles.dtype} {tiles.shape}")
        n = tiles.shape[0]
        if not 1 <= n <= self.max_batch:
            raise ValueError(f"batch {n} outside [1, {self.max_batch}]")
        d = self._dets_struct(want_probs)
        rc = self.lib.rs_engine_infer(self._h, tiles.ctypes.data_as(C.c_void_p), n, C.byref(d))
        _check(self.lib, rc, "rs_engine_infer")
        return self._collect(n, want_probs)

    # ------------------------------------------------------------------ asynchronous host interface
    def upload_async(self, tiles: np.ndarray) -> int:
        """Stage ``tiles`` in pinned memory and enqueue their upload on the engine's stream; returns the device pointer."""
        n = tiles.shape[0]
        if tiles.dtype != np.uint8 or tiles.shape[1:] != (self.tile_h, self.tile_w, self.tile_c) or not 1 <= n <= self.max_batch:
            raise ValueError(f"tiles must be uint8 (<= {self.max_batch},{self.tile_h},{self.tile_w},{self.tile_c}), got {tiles.dtype} {tiles.shape}")
        addr = tiles.ctypes.data
        if _registered_view(tiles):
            # the batch already sits in pinned memory (a registered slab, see register_host_buffer): copy straight out of it
            _check(self.lib, self.lib.rs_engine_upload_async(self._h, C.c_void_p(addr), n), "rs_engine_upload_async")
            return self.tensor_ptr("tiles")[0]
        self._stage_tiles[:n] = tiles
        _check(self.lib, self.lib.rs_engine_upload_async(self._h, self._stage_tiles.ctypes.data_as(C.c_void_p), n), "rs_engine_upload_async")
        return self.tensor_ptr("tiles")[0]

    def _crops_buffers(self) -> RsMaskCrops:
        if self._crop_data is None:
            self._crop_data = self._pinned((self.max_batch * self.D * self.tile_h * ((self.tile_w + 7) // 8),), np.uint8)
            c = RsMaskCrops()
            c.rects = self._crop_rects.ctypes.data_as(C.POINTER(C.c_int32))
            c.offsets = self._crop_offsets.ctypes.data_as(C.POINTER(C.c_uint32))
            c.data = self._crop_data.ctypes.data_as(C.POINTER(C.c_uint8))
            c.capacity = self._crop_data.nbytes
            self._crops_struct = c
        return self._crops_struct

    def fetch_async(self, n: int, crops: bool = True, polygons: bool = False, rdp_epsilon: float = 0.75, masks: bool = False) -> None:
        """Enqueue the copy of the last forward's results to the host behind it.  ``crops`` (default, with MASK_ON): the masks
        travel as crops of their boxes (``rs_mask_crops``) instead of full canvases -- 100 x h x w/8 bytes per tile shrink to
        the boxes' area, on the PCIe link and in the host-side copies.  ``polygons``: the masks are polygonised and simplified
        (``rdp_epsilon`` in pixels, <= 0: not simplified) on the device (csrc/polygonize.hip) and only the polygon tables come
        back; the ``Instances`` carry them (and the epsilon), and carry masks only with ``masks=True`` or when an instance of
        the batch exceeded the kernel's capacities and is left to the host vectoriser."""
        d = self._dets_struct(False)
        if polygons:
            if self._masks is None:
                raise RsError("polygons requested but MASK_ON is false")
            if self._poly_struct is None:
                caps = [C.c_int32() for _ in range(4)]
                self.lib.rs_polygonize_caps(*[C.byref(x) for x in caps])
                inst = self.max_batch * self.D
                self._poly_header = self._pinned((self.max_batch, self.D, POLY_HDR), np.int32)
                self._poly_prc = self._pinned((inst * caps[2].value,), np.int32)
                self._poly_rlen = self._pinned((inst * caps[2].value,), np.int32)
                self._poly_xy = self._pinned((inst * caps[1].value, 2), np.int16)
                g = RsPolygons()
                g.header = self._poly_header.ctypes.data_as(C.POINTER(C.c_int32))
                g.poly_ring_count = self._poly_prc.ctypes.data_as(C.POINTER(C.c_int32))
                g.ring_len = self._poly_rlen.ctypes.data_as(C.POINTER(C.c_int32))
                g.xy = self._poly_xy.ctypes.data_as(C.POINTER(C.c_int16))
                g.poly_cap, g.ring_cap, g.vertex_cap = self._poly_prc.size, self._poly_rlen.size, self._poly_xy.shape[0]
                g.crops = C.pointer(self._crops_buffers())
                self._poly_struct = g
            self._poly_struct.want_masks = int(bool(masks))
            self._poly_eps = max(float(rdp_epsilon), 0.0)
            d.masks = None
            _check(self.lib, self.lib.rs_engine_fetch_polygons_async(self._h, n, C.byref(d), C.byref(self._poly_struct), float(rdp_epsilon)),
                   "rs_engine_fetch_polygons_async")
            self._fetch_pending = "polygons"
        elif crops and self._masks is not None:
            d.masks = None
            _check(self.lib, self.lib.rs_engine_fetch_crops_async(self._h, n, C.byref(d), C.byref(self._crops_buffers())), "rs_engine_fetch_crops_async")
            self._fetch_pending = "crops"
        else:
            _check(self.lib, self.lib.rs_engine_fetch_async(self._h, n, C.byref(d)), "rs_engine_fetch_async")
            self._fetch_pending = "canvas"

    def wait_results(self) -> None:
        """Block until the copies of the last ``fetch_async`` have landed (for crops: wait for the crop table, copy exactly the
        bytes in use, wait for them; for polygons the same with the polygon headers and rows)."""
        kind, self._fetch_pending = self._fetch_pending or "canvas", None
        if kind == "polygons":
            _check(self.lib, self.lib.rs_engine_fetch_polygons_wait(self._h, C.byref(self._poly_struct)), "rs_engine_fetch_polygons_wait")
        elif kind == "crops":
            _check(self.lib, self.lib.rs_engine_fetch_crops_wait(self._h, C.byref(self._crops_struct)), "rs_engine_fetch_crops_wait")
        else:
            _check(self.lib, self.lib.rs_engine_fetch_wait(self._h), "rs_engine_fetch_wait")
        self._fetch_landed = kind

    def collect_results(self, n: int) -> List[Instances]:
        """``Instances`` of the results ``wait_results`` waited for (copies out of the pinned buffers)."""
        return self._collect(n, False, self._fetch_landed or "canvas")

    def fetch_wait(self, n: int) -> List[Instances]:
        self.wait_results()
        return self.collect_results(n)

    def eval_counts(self, tiles_or_n, gt_polygons: Sequence[Sequence[Sequence[np.ndarray]]]):
        """What COCO's segm matching needs of a validation batch, counted on the device: ``tiles_or_n`` = (n, h, w, c) uint8 tiles (a
        forward is run on them) or n, the batch size of the forward already enqueued; gt_polygons[tile][gt index] = list of polygons
        ([x0, y0, ...], tile pixels).  The ground truths are rasterised onto full canvases on the GPU (bit for bit
        ``rasterize_polygons_within_box(polygons, (0, 0, w, h), h)``) and no mask travels to the host.  Returns per tile
        ``(Instances without masks, inter (D_t, G_t) int32, det_area (D_t,), gt_area (G_t,))`` -- pixel counts of detection AND ground
        truth and of either alone, for ``coco_eval.match_images`` (keys mask_inter / mask_area) -- or ``None`` when the batch does
        not fit the device pool (more than 128 ground truths in a tile, max_batch * 512 polygons or max_batch * 65536 coordinates; a
        non-square tile or one above 1024 px; MASK_ON false): then nothing was run or enqueued, ``eval_fallbacks`` counts it, and the
        caller evaluates this batch from ``infer``'s masks."""
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        packed = self._eval_polygon_tables(n, gt_polygons)
        if packed is None:
            return None
        flat, off, lens, inst_first, tile_first = packed
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
        if self._eval_struct is None:
            self._eval_inter = self._pinned((self.max_batch, self.D, EVAL_GT_CAP), np.int32)
            self._eval_det_area = self._pinned((self.max_batch, self.D), np.int32)
            self._eval_gt_area = self._pinned((self.max_batch, EVAL_GT_CAP), np.int32)
            c = RsEvalCounts()
            c.inter = self._eval_inter.ctypes.data_as(C.POINTER(C.c_int32))
            c.det_area = self._eval_det_area.ctypes.data_as(C.POINTER(C.c_int32))
            c.gt_area = self._eval_gt_area.ctypes.data_as(C.POINTER(C.c_int32))
            self._eval_struct = c
        d = self._dets_struct(False)
        d.masks = None
        rc = self.lib.rs_engine_fetch_eval_async(self._h, n, C.byref(d), flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                 tile_first.ctypes.data, C.byref(self._eval_struct))
        _check(self.lib, rc, "rs_engine_fetch_eval_async")       # the fit was checked above: any other code here is an error
        _check(self.lib, self.lib.rs_engine_fetch_eval_wait(self._h), "rs_engine_fetch_eval_wait")
        out = []
        for i in range(n):
            c, g = int(self._count[i]), int(tile_first[i + 1] - tile_first[i])
            inst = Instances((self.tile_h, self.tile_w), self._boxes[i, :c].copy(), self._scores[i, :c].copy(), self._classes[i, :c].astype(np.int64),
                             None, None)
            out.append((inst, self._eval_inter[i, :c, :g].copy(), self._eval_det_area[i, :c].copy(), self._eval_gt_area[i, :g].copy()))
        return out

    def _eval_polygon_tables(self, n: int, gt_polygons, extra_unfit: bool = False):
        """The polygon tables of a validation batch as rs_engine_fetch_eval_* take them: (flat, off, lens, inst_first, tile_first), or
        ``None`` -- counted in ``eval_fallbacks`` -- when the batch does not fit the device pool (or ``extra_unfit`` says so)."""
        if len(gt_polygons) != n or not 1 <= n <= self.max_batch:
            raise ValueError(f"{len(gt_polygons)} ground-truth lists for a batch of {n} (1..{self.max_batch})")
        arrs = [np.asarray(p, np.float64).reshape(-1) for img in gt_polygons for polys in img for p in polys]
        lens = np.array([a.size for a in arrs] or [0], np.int32)
        off = np.zeros(max(len(arrs), 1), np.int64)
        if len(arrs) > 1:
            off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(1)
        inst_first = np.zeros(sum(len(img) for img in gt_polygons) + 1, np.int32)
        inst_first[1:] = np.cumsum([len(polys) for img in gt_polygons for polys in img])
        tile_first = np.zeros(n + 1, np.int32)
        tile_first[1:] = np.cumsum([len(img) for img in gt_polygons])
        rc = self.lib.rs_engine_eval_fits(self._h, n, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data, tile_first.ctypes.data)
        if rc == RS_EVAL_DOES_NOT_FIT or (rc == 0 and extra_unfit):
            self.eval_fallbacks += 1
            return None
        _check(self.lib, rc, "rs_engine_eval_fits")
        return flat, off, lens, inst_first, tile_first

    def eval_matches(self, tiles_or_n, gt_boxes: Sequence[np.ndarray], gt_classes: Sequence[np.ndarray],
                     gt_polygons: Sequence[Sequence[Sequence[np.ndarray]]], wait: bool = True):
        """``eval_counts`` and the step after it on the device: COCOeval's ``evaluateImg`` for bbox and segm (csrc/coco_match.h), behind
        the pair counts on the same stream.  gt_boxes[tile] (G_t, 4) XYXY float64 as the COCO file gives them, gt_classes[tile] (G_t,),
        gt_polygons as for ``eval_counts``; no crowd regions, no annotated areas (the caller matches such a batch on the host).  Returns
        per tile ``(Instances without masks, bbox records, segm records)``, the records being what ``coco_eval.match_images`` returns
        for that image with ``max_dets`` = the engine's slot count -- only detections and match flags travel -- or ``None`` when the
        batch does not fit (the conditions of ``eval_counts``): nothing was run or enqueued and ``eval_fallbacks`` counts it.
        ``wait=False`` returns True once everything is enqueued; ``eval_matches_wait(n)`` then gives the result."""
        from . import coco_eval
        from .coco_match import MAX_SLOTS
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        if len(gt_boxes) != n or len(gt_classes) != n:
            raise ValueError(f"{len(gt_boxes)} box lists and {len(gt_classes)} class lists for a batch of {n}")
        assert self.D == self.spec.detections_per_image       # max_dets of match_images: the cap never cuts
        packed = self._eval_polygon_tables(n, gt_polygons, extra_unfit=self.D > MAX_SLOTS)
        if packed is None:
            return None
        flat, off, lens, inst_first, tile_first = packed
        boxes = [np.asarray(b, np.float64).reshape(-1, 4) for b in gt_boxes]
        classes = [np.asarray(c, np.int32).reshape(-1) for c in gt_classes]
        if [len(b) for b in boxes] != np.diff(tile_first).tolist() or [len(c) for c in classes] != np.diff(tile_first).tolist():
            raise ValueError("ground-truth boxes, classes and polygons differ in number")
        gb = np.ascontiguousarray(np.concatenate(boxes + [np.zeros((1, 4))]))
        gc = np.ascontiguousarray(np.concatenate(classes + [np.zeros(1, np.int32)]))
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
        K, W = self.spec.num_classes, (self.D + 31) // 32
        if self._match_struct is None:
            N, T, A = self.max_batch, len(coco_eval.IOU_THRS), len(coco_eval.AREA_RNG)
            self._match_tables = {"order": self._pinned((N, self.D), np.int32), "class_first": self._pinned((N, K + 1), np.int32),
                                  "gt_per_class": self._pinned((N, K), np.int32), "matched": self._pinned((N, 2, A, T, W), np.uint32),
                                  "ignored": self._pinned((N, 2, A, T, W), np.uint32), "npig": self._pinned((N, 2, A, K), np.int32)}
            m = RsEvalMatches()
            for k, a in self._match_tables.items():
                setattr(m, k, a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_int32)))
            self._match_struct = m
        d = self._dets_struct(False)
        d.masks = None
        thr = np.ascontiguousarray(coco_eval.IOU_THRS, np.float64)
        rc = self.lib.rs_engine_fetch_eval_match_async(self._h, n, C.byref(d), flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                       tile_first.ctypes.data, gb.ctypes.data, gc.ctypes.data, thr.ctypes.data, C.byref(self._match_struct))
        _check(self.lib, rc, "rs_engine_fetch_eval_match_async")   # the fit was checked above: any other code here is an error
        return self.eval_matches_wait(n) if wait else True

    def eval_matches_wait(self, n: int):
        """The second half of ``eval_matches(..., wait=False)``: waits for the copies and builds the records of tiles 0..n-1.  Other
        work may be enqueued on the engine in between (the tables live in buffers of their own)."""
        from . import coco_eval
        from .coco_match import TABLES
        _check(self.lib, self.lib.rs_engine_fetch_eval_match_wait(self._h), "rs_engine_fetch_eval_match_wait")
        t0 = time.perf_counter()
        out = []
        for i in range(n):
            c = int(self._count[i])
            inst = Instances((self.tile_h, self.tile_w), self._boxes[i, :c].copy(), self._scores[i, :c].copy(), self._classes[i, :c].astype(np.int64),
                             None, None)
            t = [self._match_tables[k][i].copy() for k in TABLES]
            out.append((inst, coco_eval.records_from_tables(self._scores[i].copy(), *t, iou_type="bbox"),
                        coco_eval.records_from_tables(self._scores[i].copy(), *t, iou_type="segm")))
        self.eval_unpack_s += time.perf_counter() - t0       # host time of this route's matching: unpacking the flag bits
        return out

    def road_votes(self, tiles_or_n, labels: Sequence[Sequence[Sequence[np.ndarray]]], threshold: float = 0.0, wait: bool = True,
                   geometry: str = "pixels", rdp_epsilon: float = 0.75):
        """The road cover vote of a batch, counted and summed on the device (csrc/road_vote.h): ``tiles_or_n`` as for ``eval_counts``
        (tiles: a forward is run on them; n: the forward already enqueued, whether or not a ``fetch_async`` of it is in flight);
        labels[tile][label] = list of rings ([x0, y0, x1, y1, ...], tile pixels), the road labels clipped to the tile.  The labels are
        rasterised on the GPU exactly as ``raster_vote.label_rasters`` does on the host, and neither a mask nor a pair count travels.
        Returns per tile ``(Instances without masks, wscore (L_t, K) float64, wfrac (L_t, K) float64, pairs (L_t, K) int32, label_area
        (L_t,) int32)`` -- per label and class the sum of weighted scores, the sum of weights and the number of (label, detection) pairs
        with ``score >= threshold``; ``raster_vote.reduce_votes`` turns them into the road table -- or ``None`` when the batch does not
        fit the device pool (the conditions of ``eval_counts``, shared with it; also more than 1024 slots): then nothing was enqueued,
        nothing is truncated, ``vote_fallbacks`` counts it and the caller votes on this batch with ``raster_vote.vote_tables_host``.
        Without a ``fetch_async`` in flight the detections (no masks) are fetched too; with one, its copies bring them.
        ``wait=False`` returns True once everything is enqueued; ``road_votes_wait(n)`` then gives the result.
        ``geometry="polygons"``: the weights are areas of polygon intersections (``road_votes_polygons``; T = 1, the threshold axis
        dropped, ``label_area`` float64, the ``Instances`` carry the polygons); ``wait=False`` then pairs with ``road_votes_polygons_wait``."""
        from .raster_vote import check_vote_geometry
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        if not np.isfinite(threshold):                # before the forward: a refused call enqueues nothing
            raise ValueError(f"vote threshold {threshold!r} is not finite")
        if check_vote_geometry(geometry) == "polygons":
            return self.road_votes_polygons(tiles_or_n, labels, [threshold], wait=wait, rdp_epsilon=rdp_epsilon, squeeze=True)
        packed = self._vote_label_tables(n, labels)
        if packed is None:
            return None
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
        self._vote_labels = self._vote_enqueue(n, packed, threshold)
        return self.road_votes_wait(n) if wait else True

    def _vote_label_tables(self, n: int, labels):
        """The label tables of a batch as rs_engine_fetch_votes_async takes them, or ``None`` -- counted in ``vote_fallbacks`` -- when the
        batch does not fit the device pool.  The pool and its check are those of the validation counts; the counters are not."""
        from .coco_match import MAX_SLOTS
        before = self.eval_fallbacks
        packed = self._eval_polygon_tables(n, labels, extra_unfit=self.D > MAX_SLOTS)
        self.eval_fallbacks = before
        if packed is None:
            self.vote_fallbacks += 1
        return packed

    def _vote_enqueue(self, n: int, packed, threshold: float) -> List[int]:
        """Enqueue the vote of ``_vote_label_tables``' tables behind the last forward (and behind its fetch, when one is in flight);
        returns the labels per tile."""
        if not np.isfinite(threshold):
            raise ValueError(f"vote threshold {threshold!r} is not finite")
        flat, off, lens, inst_first, tile_first = packed
        if self._fetch_pending is None:               # no fetch of this forward in flight: bring the detections (no masks) along
            d = self._dets_struct(False)
            d.masks = None
            _check(self.lib, self.lib.rs_engine_fetch_async(self._h, n, C.byref(d)), "rs_engine_fetch_async")
        K = self.spec.num_classes
        if self._vote_struct is None:
            self._vote_tables = {"wscore": self._pinned((self.max_batch, EVAL_GT_CAP, K), np.float64),
                                 "wfrac": self._pinned((self.max_batch, EVAL_GT_CAP, K), np.float64),
                                 "pairs": self._pinned((self.max_batch, EVAL_GT_CAP, K), np.int32),
                                 "label_area": self._pinned((self.max_batch, EVAL_GT_CAP), np.int32)}
            v = RsRoadVotes()
            for k, a in self._vote_tables.items():
                setattr(v, k, a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int32)))
            self._vote_struct = v
        rc = self.lib.rs_engine_fetch_votes_async(self._h, n, flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                  tile_first.ctypes.data, float(threshold), C.byref(self._vote_struct))
        _check(self.lib, rc, "rs_engine_fetch_votes_async")        # the fit was checked above: any other code here is an error
        return np.diff(tile_first).tolist()

    def road_votes_wait(self, n: int, with_instances: bool = True, label_counts: Optional[Sequence[int]] = None):
        """The second half of ``road_votes(..., wait=False)``: waits for the copies and returns the tables of tiles 0..n-1.  A
        ``fetch_async`` of the same forward that is in flight keeps its own ``wait_results``, before or after this call.
        ``with_instances=False`` leaves the detections to that fetch and gives ``(wscore, wfrac, pairs, label_area)`` per tile.
        ``label_counts``: the labels per tile of the batch the tables belong to, for a caller that has enqueued another since."""
        _check(self.lib, self.lib.rs_engine_fetch_votes_wait(self._h), "rs_engine_fetch_votes_wait")
        t = self._vote_tables
        counts = self._vote_labels if label_counts is None else label_counts
        out = []
        for i in range(n):
            g = int(counts[i])
            row = (t["wscore"][i, :g].copy(), t["wfrac"][i, :g].copy(), t["pairs"][i, :g].copy(), t["label_area"][i, :g].copy())
            if with_instances:
                c = int(self._count[i])
                row = (Instances((self.tile_h, self.tile_w), self._boxes[i, :c].copy(), self._scores[i, :c].copy(),
                                 self._classes[i, :c].astype(np.int64), None, None),) + row
            out.append(row)
        return out

    def road_votes_sweep(self, tiles_or_n, labels: Sequence[Sequence[Sequence[np.ndarray]]], thresholds, wait: bool = True,
                         geometry: str = "pixels", rdp_epsilon: float = 0.75):
        """``road_votes`` for a list of 1 to 32 finite score thresholds at once (csrc/road_vote.h, THE SWEEP): labels are uploaded,
        rasterised and counted once, ``road_vote_sweep_kernel`` forms the tables of every threshold, and only they travel.  Returns
        per tile ``(Instances without masks, wscore (T, L_t, K), wfrac (T, L_t, K), pairs (T, L_t, K), label_area (L_t,))``; slice j
        has the bits of ``road_votes`` at ``thresholds[j]`` (``raster_vote.sweep_slice`` gives it to ``reduce_votes``).  ``None``
        when the batch does not fit the device pool, under the conditions of ``road_votes`` and counted in ``vote_fallbacks`` like
        there: sweep that batch with ``raster_vote.vote_tables_host(..., thresholds=)``.  ``wait=False`` returns True once
        everything is enqueued; ``road_votes_sweep_wait(n)`` then gives the result."""
        from .raster_vote import check_vote_geometry, sweep_thresholds
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        thr = sweep_thresholds(thresholds)            # before the forward: a refused call enqueues nothing
        if check_vote_geometry(geometry) == "polygons":
            return self.road_votes_polygons(tiles_or_n, labels, thr, wait=wait, rdp_epsilon=rdp_epsilon)
        packed = self._vote_label_tables(n, labels)
        if packed is None:
            return None
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
        self._sweep_labels = self._sweep_enqueue(n, packed, thr)
        return self.road_votes_sweep_wait(n) if wait else True

    # ------------------------------------------------------------------ the vote on polygon areas (csrc/poly_overlap.h)
    def road_votes_polygons(self, tiles_or_n, labels: Sequence[Sequence[Sequence[np.ndarray]]], thresholds, wait: bool = True,
                            rdp_epsilon: float = 0.75, squeeze: bool = False):
        """The vote of ``road_votes_sweep`` with the reference's geometry: a (label, detection) pair weighs
        ``round(area(label ∩ detection polygons) / area(label), 2)``, both areas on polygons -- the detection's as the device
        polygoniser made them (simplified with ``rdp_epsilon``, the ones that go into the GeoPackage), the label's rings as given
        (every ring an exterior; simple and pairwise interior-disjoint, which is not checked).  It rides behind a polygons fetch of
        the same forward: with tiles, or with n and no fetch in flight, ``fetch_async(n, polygons=True, rdp_epsilon=...)`` is
        enqueued here; a polygons fetch already in flight is used as it is (its epsilon counts); another kind of fetch in flight
        is a ``ValueError``.  Neither the rasteriser nor the pair counts run.  Returns per tile ``(Instances with polygons, wscore
        (T, L_t, K), wfrac, pairs, label_area (L_t,) float64)``, or ``None`` -- nothing enqueued, ``vote_fallbacks`` counted -- when
        the batch does not fit the device pool: vote on it with ``raster_vote.vote_tables_polygons_host``.  A batch in which the
        polygoniser flagged an instance comes back through that host route by itself (after the host vectoriser has made the
        flagged instance's polygons), also counted in ``vote_fallbacks``.  ``squeeze``: T = 1 and the threshold axis dropped.
        ``wait=False`` returns True once everything is enqueued; ``road_votes_polygons_wait(n)`` then gives the result and
        completes the polygons fetch (use ``collect_results``, not ``wait_results``, after it)."""
        from .raster_vote import sweep_thresholds
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        thr = sweep_thresholds(thresholds)            # before the forward: a refused call enqueues nothing
        if np.isscalar(tiles_or_n) and self._fetch_pending not in (None, "polygons"):
            raise ValueError(f"the vote geometry 'polygons' rides behind a polygons fetch, a {self._fetch_pending} fetch is in flight")
        packed = self._vote_label_tables(n, labels)
        if packed is None:
            return None
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
            self._fetch_pending = None
        if self._fetch_pending is None:
            self.fetch_async(n, polygons=True, rdp_epsilon=rdp_epsilon)
        self._pvote_labels = self._pvote_enqueue(n, packed, thr)
        self._pvote_batch = (labels, thr, bool(squeeze))
        return self.road_votes_polygons_wait(n) if wait else True

    def _pvote_enqueue(self, n: int, packed, thresholds) -> Tuple[List[int], int]:
        """Enqueue the polygon vote of ``_vote_label_tables``' tables behind the polygons fetch of the last forward that is in flight;
        returns (the labels per tile, the number of thresholds)."""
        from .raster_vote import sweep_thresholds
        thr = sweep_thresholds(thresholds)
        flat, off, lens, inst_first, tile_first = packed
        K = self.spec.num_classes
        if self._pvote_struct is None:
            cells = self.max_batch * VOTE_SWEEP_MAX * EVAL_GT_CAP * K      # flat: the layout [n][T][cap][K] depends on the call's n and T
            self._pvote_tables = {"wscore": self._pinned((cells,), np.float64), "wfrac": self._pinned((cells,), np.float64),
                                  "pairs": self._pinned((cells,), np.int32),
                                  "label_area": self._pinned((self.max_batch, EVAL_GT_CAP), np.float64),
                                  "flagged": self._pinned((self.max_batch,), np.int32)}
            v = RsRoadVotesPoly()
            for k, a in self._pvote_tables.items():
                setattr(v, k, a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int32)))
            self._pvote_struct = v
        rc = self.lib.rs_engine_fetch_votes_poly_async(self._h, n, flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                       tile_first.ctypes.data, thr.ctypes.data, int(thr.size), C.byref(self._pvote_struct))
        _check(self.lib, rc, "rs_engine_fetch_votes_poly_async")   # the fit was checked above: any other code here is an error
        return np.diff(tile_first).tolist(), int(thr.size)

    def _pvote_wait(self, n: int, label_counts=None):
        """Waits for the polygon vote's copies; the rows ``(wscore (T, L_t, K), wfrac, pairs, label_area)`` of tiles 0..n-1, or ``None``
        when the polygoniser flagged an instance of the batch: its pairs were left at zero, the batch takes the host route."""
        _check(self.lib, self.lib.rs_engine_fetch_votes_poly_wait(self._h), "rs_engine_fetch_votes_poly_wait")
        if int(self._pvote_tables["flagged"][:n].sum()):
            return None
        counts, T = self._pvote_labels if label_counts is None else label_counts
        K = self.spec.num_classes
        t = {k: self._pvote_tables[k][:n * T * EVAL_GT_CAP * K].reshape(n, T, EVAL_GT_CAP, K) for k in ("wscore", "wfrac", "pairs")}
        return [(t["wscore"][i, :, :int(counts[i])].copy(), t["wfrac"][i, :, :int(counts[i])].copy(), t["pairs"][i, :, :int(counts[i])].copy(),
                 self._pvote_tables["label_area"][i, :int(counts[i])].copy()) for i in range(n)]

    def polygon_vote_host_rows(self, inst: Sequence[Instances], labels, thresholds):
        """The host route of the polygon vote on fetched ``Instances`` that carry polygons (and the crops of flagged instances, which
        the host vectoriser turns into polygons first): ``raster_vote.vote_tables_polygons_host``'s rows."""
        from .raster_vote import vote_tables_polygons_host
        from .vectorize import vectorize_masks_native
        lists = [vectorize_masks_native(None, self.tile_h, self.tile_w, i._polygons.rdp_epsilon, polygons=i._polygons, crops=i._crops) for i in inst]
        return vote_tables_polygons_host(lists, labels, [i.scores for i in inst], [i.pred_classes for i in inst], thresholds, self.spec.num_classes)

    def road_votes_polygons_wait(self, n: int):
        """The second half of ``road_votes_polygons(..., wait=False)``: waits for the vote's copies and for the polygons fetch it
        rides behind, and returns the rows of tiles 0..n-1.  A batch with a flagged instance is voted again on the host."""
        rows = self._pvote_wait(n)
        if self._fetch_pending == "polygons":
            self.wait_results()
        inst = self.collect_results(n)
        labels, thr, squeeze = self._pvote_batch
        if rows is None:
            self.vote_fallbacks += 1
            rows = self.polygon_vote_host_rows(inst, labels, thr)
        if squeeze:
            rows = [(r[0][0], r[1][0], r[2][0], r[3]) for r in rows]
        return [(i,) + tuple(r) for i, r in zip(inst, rows)]

    def _sweep_enqueue(self, n: int, packed, thresholds) -> Tuple[List[int], int]:
        """Enqueue the sweep of ``_vote_label_tables``' tables behind the last forward (and behind its fetch, when one is in flight);
        returns (the labels per tile, the number of thresholds)."""
        from .raster_vote import sweep_thresholds
        thr = sweep_thresholds(thresholds)
        flat, off, lens, inst_first, tile_first = packed
        if self._fetch_pending is None:               # no fetch of this forward in flight: bring the detections (no masks) along
            d = self._dets_struct(False)
            d.masks = None
            _check(self.lib, self.lib.rs_engine_fetch_async(self._h, n, C.byref(d)), "rs_engine_fetch_async")
        K = self.spec.num_classes
        if self._sweep_struct is None:
            cells = self.max_batch * VOTE_SWEEP_MAX * EVAL_GT_CAP * K      # flat: the layout [n][T][cap][K] depends on the call's n and T
            self._sweep_tables = {"wscore": self._pinned((cells,), np.float64), "wfrac": self._pinned((cells,), np.float64),
                                  "pairs": self._pinned((cells,), np.int32),
                                  "label_area": self._pinned((self.max_batch, EVAL_GT_CAP), np.int32)}
            v = RsRoadVoteSweep()
            for k, a in self._sweep_tables.items():
                setattr(v, k, a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_int32)))
            self._sweep_struct = v
        rc = self.lib.rs_engine_fetch_vote_sweep_async(self._h, n, flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                       tile_first.ctypes.data, thr.ctypes.data, int(thr.size), C.byref(self._sweep_struct))
        _check(self.lib, rc, "rs_engine_fetch_vote_sweep_async")   # the fit was checked above: any other code here is an error
        return np.diff(tile_first).tolist(), int(thr.size)

    def road_votes_sweep_wait(self, n: int, with_instances: bool = True, label_counts=None):
        """The second half of ``road_votes_sweep(..., wait=False)``, as ``road_votes_wait`` is of ``road_votes``.  ``label_counts``:
        what ``_sweep_enqueue`` returned for the batch the tables belong to, for a caller that has enqueued another since."""
        _check(self.lib, self.lib.rs_engine_fetch_vote_sweep_wait(self._h), "rs_engine_fetch_vote_sweep_wait")
        counts, T = self._sweep_labels if label_counts is None else label_counts
        K = self.spec.num_classes
        t = {k: a[:n * T * EVAL_GT_CAP * K].reshape(n, T, EVAL_GT_CAP, K) for k, a in self._sweep_tables.items() if k != "label_area"}
        out = []
        for i in range(n):
            g = int(counts[i])
            row = (t["wscore"][i, :, :g].copy(), t["wfrac"][i, :, :g].copy(), t["pairs"][i, :, :g].copy(),
                   self._sweep_tables["label_area"][i, :g].copy())
            if with_instances:
                c = int(self._count[i])
                row = (Instances((self.tile_h, self.tile_w), self._boxes[i, :c].copy(), self._scores[i, :c].copy(),
                                 self._classes[i, :c].astype(np.int64), None, None),) + row
            out.append(row)
        return out

    def band_hist(self, tiles_or_n, labels: Sequence[Sequence[Sequence[np.ndarray]]], wait: bool = True):
        """The band histograms under the road labels of a batch, counted on the device (csrc/band_hist.h): ``tiles_or_n`` and ``labels``
        as for ``road_votes``.  The labels are rasterised on the GPU exactly as ``raster_vote.label_rasters`` does on the host and
        counted against the uint8 tiles of the forward; only the histograms travel.  Returns per tile an ``(L_t, C, 256)`` uint32
        array -- per label, band and value the number of the label's pixels that are not nodata (every band 0);
        ``band_stats.reduce_band_hist`` and ``stats_from_hist`` turn them into the reference's table -- or ``None`` when the batch does
        not fit the device pool (the conditions of ``eval_counts``, shared with it): then nothing was enqueued, ``band_fallbacks``
        counts it and the caller uses ``band_stats.band_hist_host`` on this batch.  It carries no detections and may follow any
        ``fetch_async`` and ``road_votes(..., wait=False)`` of the same forward.  ``wait=False`` returns True once everything is
        enqueued; ``band_hist_wait(n)`` then gives the result, and tiles uploaded in between are ordered behind the kernel."""
        n = int(tiles_or_n) if np.isscalar(tiles_or_n) else int(tiles_or_n.shape[0])
        packed = self._band_label_tables(n, labels)
        if packed is None:
            return None
        if not np.isscalar(tiles_or_n):
            self.infer_device(self.upload_async(np.ascontiguousarray(tiles_or_n)), n)
        self._band_labels = self._band_enqueue(n, packed)
        return self.band_hist_wait(n) if wait else True

    def _band_label_tables(self, n: int, labels):
        """The label tables of a batch as rs_engine_fetch_band_hist_async takes them, or ``None`` -- counted in ``band_fallbacks`` --
        when the batch does not fit the device pool.  The pool and its check are those of the validation counts; the counters are not."""
        before = self.eval_fallbacks
        packed = self._eval_polygon_tables(n, labels)
        self.eval_fallbacks = before
        if packed is None:
            self.band_fallbacks += 1
        return packed

    def _band_enqueue(self, n: int, packed) -> List[int]:
        """Enqueue the histograms of ``_band_label_tables``' tables behind the last forward (and behind whatever fetch of it is in
        flight); returns the labels per tile."""
        flat, off, lens, inst_first, tile_first = packed
        if self._band_struct is None:
            self._band_table = self._pinned((self.max_batch * EVAL_GT_CAP, self.tile_c, 256), np.uint32)
            b = RsBandHist()
            b.hist = self._band_table.ctypes.data_as(C.POINTER(C.c_uint32))
            self._band_struct = b
        rc = self.lib.rs_engine_fetch_band_hist_async(self._h, n, flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                                      tile_first.ctypes.data, C.byref(self._band_struct))
        _check(self.lib, rc, "rs_engine_fetch_band_hist_async")    # the fit was checked above: any other code here is an error
        self._band_pending = True
        return np.diff(tile_first).tolist()

    def band_hist_wait(self, n: int, label_counts: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        """The second half of ``band_hist(..., wait=False)``: waits for the copy and returns the histograms of tiles 0..n-1.  A
        ``fetch_async`` of the same forward that is in flight keeps its own ``wait_results``, before or after this call.
        ``label_counts``: the labels per tile of the batch the table belongs to, for a caller that has enqueued another since."""
        _check(self.lib, self.lib.rs_engine_fetch_band_hist_wait(self._h), "rs_engine_fetch_band_hist_wait")
        self._band_pending = False
        counts = self._band_labels if label_counts is None else label_counts
        out, g0 = [], 0
        for i in range(n):
            g = int(counts[i])
            out.append(self._band_table[g0:g0 + g].copy())
            g0 += g
        return out

    def infer_device(self, tiles_dev_ptr: int, n: int) -> None:
        """Enqueue a forward on tiles already in device memory (no wait)."""
        _check(self.lib, self.lib.rs_engine_infer_device(self._h, C.c_void_p(tiles_dev_ptr), n), "rs_engine_infer_device")

    def infer_phase(self, tiles_dev_ptr: int, n: int, phase: int) -> None:
        """Enqueue one phase (0, 1, 2) of a forward; see ``LanePipeline`` and include/rs_engine.h."""
        _check(self.lib, self.lib.rs_engine_infer_phase(self._h, C.c_void_p(tiles_dev_ptr), n, phase), "rs_engine_infer_phase")

    def sync(self) -> None:
        _check(self.lib, self.lib.rs_engine_sync(self._h), "rs_engine_sync")

    def fetch(self, n: int, want_probs: bool = False) -> List[Instances]:
        d = self._dets_struct(want_probs)
        _check(self.lib, self.lib.rs_engine_fetch(self._h, n, C.byref(d)), "rs_engine_fetch")
        return self._collect(n, want_probs)

    @property
    def stream(self) -> int:
        return int(self.lib.rs_engine_stream(self._h) or 0)

    def net_shape(self) -> Tuple[int, int, int, int]:
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib, self.lib.rs_engine_net_shape(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "net_shape")
        return a.value, b.value, c.value, d.value

    # ------------------------------------------------------------------ introspection
    def tensor_names(self) -> List[str]:
        buf = C.create_string_buffer(96)
        names = []
        for i in range(self.lib.rs_engine_tensor_count(self._h)):
            self.lib.rs_engine_tensor_name(self._h, i, buf)
            names.append(buf.value.decode())
        return names

    def tensor_ptr(self, name: str) -> Tuple[int, np.dtype, Tuple[int, ...], int]:
        p, dt, nd, halo = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        dims = (C.c_int64 * 5)()
        _check(self.lib, self.lib.rs_engine_tensor(self._h, name.encode(), C.byref(p), C.byref(dt), C.byref(nd), dims, C.byref(halo)),
               f"rs_engine_tensor({name})")
        return int(p.value), np.dtype(DT_NP[dt.value]), tuple(int(dims[i]) for i in range(nd.value)), halo.value

    def tensor(self, name: str, n: Optional[int] = None, strip_halo: bool = True) -> np.ndarray:
        """Copy an intermediate tensor to the host.  NHWC activations lose their halo; ``n`` limits the
        leading (batch) dimension."""
        ptr, dt, shape, halo = self.tensor_ptr(name)
        if self.tensor_is_split(name):
            # split-operand mode: two fp16 planes of the full shape back to back; fp32(hi) + fp32(lo) is exact
            planes = np.empty((2,) + shape, np.float16)
            _check(self.lib, self.lib.rs_memcpy_d2h(planes.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), planes.nbytes), "rs_memcpy_d2h")
            a = planes[0].astype(np.float32) + planes[1].astype(np.float32)
            if n is not None:
                a = a[: min(n, shape[0])]
        else:
            if n is not None:
                shape = (min(n, shape[0]),) + shape[1:]
            a = np.empty(shape, dt)
            _check(self.lib, self.lib.rs_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes), "rs_memcpy_d2h")
        if strip_halo and halo:
            a = a[:, halo:-halo, halo:-halo]
        return a

    def tensor_is_split(self, name: str) -> bool:
        dt = C.c_int32()
        _check(self.lib, self.lib.rs_engine_tensor(self._h, name.encode(), None, C.byref(dt), None, None, None), f"rs_engine_tensor({name})")
        return dt.value == DT_SPLIT16

    def set_profiling(self, mode: int) -> None:
        """0 off, 1 per-stage events + host wait, 2 events only (read back by ``stage_times``)."""
        _check(self.lib, self.lib.rs_engine_set_profiling(self._h, int(mode)), "rs_engine_set_profiling")

    def upload_tiles(self, tiles: np.ndarray) -> int:
        """Copy tiles into the engine's own device input buffer; returns its device pointer so that
        ``infer_device`` can run on tiles already resident in HBM (no staging copy)."""
        tiles = np.ascontiguousarray(tiles)
        assert tiles.dtype == np.uint8 and tiles.shape[1:] == (self.tile_h, self.tile_w, self.tile_c) and tiles.shape[0] <= self.max_batch
        ptr, _, _, _ = self.tensor_ptr("tiles")
        if self._band_pending:               # this copy is on no stream of the engine's: let the histogram kernel finish with the tiles first
            _check(self.lib, self.lib.rs_engine_fetch_band_hist_wait(self._h), "rs_engine_fetch_band_hist_wait")
            self._band_pending = False
        _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(ptr), tiles.ctypes.data_as(C.c_void_p), tiles.nbytes), "rs_memcpy_h2d")
        return ptr

    def stage_times(self) -> List[Dict[str, Any]]:
        out = []
        name = C.create_string_buffer(96)
        ms, fl, by, calls = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        for i in range(self.lib.rs_engine_stage_count(self._h)):
            self.lib.rs_engine_stage_info(self._h, i, name, C.byref(ms), C.byref(calls), C.byref(fl), C.byref(by))
            kn = C.create_string_buffer(96)
            self.lib.rs_engine_stage_kernel(self._h, i, kn)
            out.append({"name": name.value.decode(), "ms_total": ms.value, "calls": calls.value, "flops": fl.value, "bytes": by.value,
                        "kernel": kn.value.decode()})
        return out

    def saturation(self) -> Dict[str, int]:
        """Elements clamped to the fp16 range, by stage, in the most recent forward whose results were fetched (``infer``, ``fetch``,
        ``wait_results`` / ``fetch_wait``); stages with a zero count are left out."""
        n = self.lib.rs_engine_stage_count(self._h)
        counts = np.zeros(max(n, 1), np.int64)
        rc = self.lib.rs_engine_saturation(self._h, counts.ctypes.data_as(C.POINTER(C.c_int64)), n)
        if rc < 0:
            _check(self.lib, rc, "rs_engine_saturation")
        names = getattr(self, "_stage_names", None)
        if names is None or len(names) != n:
            buf = C.create_string_buffer(96)
            names = []
            for i in range(n):
                self.lib.rs_engine_stage_info(self._h, i, buf, None, None, None, None)
                names.append(buf.value.decode())
            self._stage_names = names
        out: Dict[str, int] = {}
        for i in np.flatnonzero(counts[:n]):
            out[names[i]] = out.get(names[i], 0) + int(counts[i])
        return out

    def stage_variants(self) -> Dict[str, int]:
        """Conv tile variant each GEMM stage launched in its last call (numbering: include/rs_engine.h rs_op_conv_variant)."""
        name = C.create_string_buffer(96)
        out = {}
        for i in range(self.lib.rs_engine_stage_count(self._h)):
            v = self.lib.rs_engine_stage_variant(self._h, i)
            if v != -2:
                self.lib.rs_engine_stage_info(self._h, i, name, None, None, None, None)
                out[name.value.decode()] = v
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.rs_engine_destroy(self._h)
            self._h = None
            self._crops_struct = None
            for name in ("_count", "_boxes", "_scores", "_classes", "_masks", "_stage_tiles", "_crop_rects", "_crop_offsets", "_crop_data"):
                setattr(self, name, None)             # views over the pinned memory freed below
            for p in getattr(self, "_pinned_ptrs", []):
                self.lib.rs_host_free(p)
            self._pinned_ptrs = []

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


VECTORIZE_MODES = ("host", "device")


class LanePipeline:
    """Several engines ("lanes") fed alternately so that consecutive batches overlap on one GPU.  The reference processes one tile at a time
    and has no counterpart ([EXT d2: engine/defaults.py]).  Two forms:

    * independent lanes (default since the end of round 4): every lane is a complete engine on its OWN stream and a batch is one ``infer_device``
      on its lane; the hardware interleaves the workgroups of the lanes' kernels.  On one stream every CU reaches the HBM-bound prologue / epilogue of
      a ``conv_deep`` tile together and the matrix pipe idles meanwhile; kernels of two queues run out of phase, and one lane's
      latency-bound detection glue runs beside the other's convolutions.  Against the phased form (``tools/ubench/two_pipes.py``, one box): split mode
      905 -> 954 tiles/s at batch 16, 821 -> 891 at batch 8; fp16 2 189 -> 2 241 and 1 796 -> 2 068.  Bit-identical to a single engine -- once the
      device code stopped using the compiler's fp32 division sequence, which returns wrong quotients beside another kernel's MFMA waves
      (csrc/common.h ``rs_fdiv``; ``tools/parity/lanes_stress.py``: 8 400 tile results, none differing).
    * ``shared_stream=True`` (rounds 2-4): the lanes' convolutions serialised on ONE wide stream, each lane's glue on its own side stream
      behind the other lane's convolutions.  Enqueue order for batch k on lane k mod 2:

          phase0(k)   backbone, FPN, RPN heads  -> glue G1(k) on the side stream
          phase2(k-1) mask head of the previous batch (hides G1(k))
          phase1(k)   box head                  -> glue G2(k) on the side stream, hidden by phase0(k+1)

      Results of batch k are complete once phase2(k) has run, i.e. after ``submit`` of batch k+1 or ``flush``."""

    def __init__(self, spec: EngineSpec, weights: Dict[str, np.ndarray], tile_shape: Tuple[int, int, int], max_batch: int = 16,
                 device: int = 0, lanes: int = 2, shared_stream: bool = False, vectorize: str = "host", rdp_epsilon: float = 0.75):
        if lanes not in (1, 2, 3, 4):
            raise ValueError("lanes must be 1..4")
        if vectorize not in VECTORIZE_MODES:
            raise ValueError(f"vectorize must be one of {VECTORIZE_MODES}, got {vectorize!r}")
        # "device": ``run`` fetches polygons traced and simplified on the GPU (Engine.fetch_async(polygons=True)) instead of mask crops;
        # ``want_masks`` makes those batches bring their masks too
        self.vectorize, self.rdp_epsilon, self.want_masks = vectorize, float(rdp_epsilon), False
        blob = pack_weights(spec, weights)           # folding + fragment orders once, not once per lane (0.3 s of host time each)
        self.shared = bool(shared_stream) and lanes > 1
        first = Engine(spec, weights, tile_shape, max_batch, device, blob=blob)
        self.engines = [first] + [Engine(spec, weights, tile_shape, max_batch, device, stream=first.stream if self.shared else None, blob=blob)
                                  for _ in range(lanes - 1)]
        self.k = 0
        self._pending: Optional[Tuple[int, int, int]] = None     # shared form: (lane, tiles ptr, n) whose phase 2 is still to be enqueued
        # saturation counts (Engine.saturation) of the batch ``run`` yielded last: set before the batch is yielded
        self.last_saturation: Dict[str, int] = {}
        self.vote_fallbacks = 0                      # batches of the last ``run(..., labels=...)`` that were voted on the host
        self.band_fallbacks = 0                      # batches of the last ``run(..., band_stats=True)`` whose histograms the host formed

    def _fetch_async(self, e: Engine, n: int, masks: bool = False) -> None:
        if self.vectorize == "device" and e.spec.mask_on:
            e.fetch_async(n, polygons=True, rdp_epsilon=self.rdp_epsilon, masks=self.want_masks or masks)
        else:
            e.fetch_async(n)

    def lane_of_next(self) -> Engine:
        return self.engines[self.k % len(self.engines)]

    def submit(self, tiles_dev_ptr: int, n: int) -> int:
        """Enqueue one batch (tiles resident in the next lane's device memory); returns the lane index used."""
        lane = self.k % len(self.engines)
        e = self.engines[lane]
        self.k += 1
        if not self.shared:
            e.infer_device(tiles_dev_ptr, n)
            return lane
        e.infer_phase(tiles_dev_ptr, n, 0)
        self._finish_pending()
        e.infer_phase(tiles_dev_ptr, n, 1)
        self._pending = (lane, tiles_dev_ptr, n)
        return lane

    def _finish_pending(self) -> None:
        if self._pending is not None:
            lane, ptr, n = self._pending
            self.engines[lane].infer_phase(ptr, n, 2)
            self._pending = None

    def flush(self) -> None:
        """Enqueue the outstanding mask-head phase; after this every submitted batch is fully enqueued."""
        self._finish_pending()

    def run(self, batches, labels=None, vote_threshold: float = 0.0, band_stats: bool = False, road_votes: bool = True,
            vote_sweep=None, vote_geometry: str = "pixels") -> "Iterator[List[Instances]]":
        """Stream host batches ((n,h,w,c) uint8 arrays) through the lanes and yield their detections in order.  Uploads go
        through pinned staging on the lane's stream, every batch's results come back on its lane's copy stream behind an event,
        and the generator runs ``lanes`` batches ahead of what it yields, so host-side collection overlaps the GPU.  Independent lanes:
            submit(k): upload(k), forward(k), fetch_async(k);   then collect + yield batch k - lanes
        shared stream:
            submit(k): upload(k), phase0(k), phase2(k-1) + fetch_async(k-1), phase1(k);   then collect + yield batch k-2.
        ``labels``: an iterable parallel to ``batches``, per batch the road labels of its tiles as ``Engine.road_votes`` takes them.
        Then every yielded ``Instances`` carries ``road_votes`` = (wscore, wfrac, pairs, label_area) of its tile: the vote fetch is
        enqueued right behind the batch's result fetch on the batch's lane, and a batch that does not fit the device pool is fetched
        with its masks and voted on the host (``raster_vote.vote_tables_host``), counted in ``vote_fallbacks``.
        ``band_stats=True`` (needs ``labels``): every yielded ``Instances`` also carries ``band_hist``, the (L_t, C, 256) histograms of
        its tile's labels (``Engine.band_hist``), enqueued behind the batch's other fetches on its lane; a batch that does not fit gets
        them from ``band_stats.band_hist_host`` on its own host tiles, which the pipeline keeps until the batch is yielded, counted in
        ``band_fallbacks``.  ``road_votes=False`` leaves the vote out: labels then serve the histograms alone.
        ``vote_sweep=thresholds`` (needs ``labels``; 1 to 32 finite values): every yielded ``Instances`` also carries
        ``road_vote_sweep`` = (wscore (T, L, K), wfrac, pairs, label_area) of its tile (``Engine.road_votes_sweep``), swept on the host
        (``vote_tables_host(..., thresholds=)``) for a batch that does not fit, counted in ``vote_fallbacks``.  With ``road_votes``
        as well the pipeline runs the sweep alone, ``vote_threshold`` appended as its last entry (so at most 31 thresholds then), and
        sets ``road_votes`` from that slice -- slice j of a sweep has the bits of the vote at ``thresholds[j]`` (csrc/road_vote.h) --
        so the rasteriser and the pair counts run once per batch, not twice.
        ``vote_geometry="polygons"`` (needs ``vectorize="device"``, refused before any forward otherwise): the weights of both are areas
        of polygon intersections (csrc/poly_overlap.h, ``Engine.road_votes_polygons``) on the polygons of the batch's own fetch; neither
        the rasteriser nor the pair counts run, ``label_area`` is float64.  A batch with a flagged instance, and one that does not fit
        the pool, is voted on the host (``raster_vote.vote_tables_polygons_host``), counted in ``vote_fallbacks``."""
        from .raster_vote import check_vote_geometry
        poly_geo = check_vote_geometry(vote_geometry, self.vectorize) == "polygons"
        if poly_geo and not self.engines[0].spec.mask_on:
            raise ValueError("the vote geometry 'polygons' needs MASK_ON")
        if band_stats and labels is None:
            raise ValueError("band_stats needs the road labels of every batch")
        if vote_sweep is not None and labels is None:
            raise ValueError("vote_sweep needs the road labels of every batch")
        want_votes = labels is not None and bool(road_votes)
        sweep_all, sweep_T = None, 0                # the list the sweep runs on (vote_threshold behind the caller's), the caller's length
        if vote_sweep is not None:
            from .raster_vote import sweep_thresholds
            sweep_all = sweep_thresholds(vote_sweep)
            sweep_T = int(sweep_all.size)
            if want_votes:
                if not np.isfinite(vote_threshold):
                    raise ValueError(f"vote threshold {vote_threshold!r} is not finite")
                if sweep_T >= VOTE_SWEEP_MAX:
                    raise ValueError(f"vote_sweep with road_votes takes at most {VOTE_SWEEP_MAX - 1} thresholds: the vote's own is appended")
                sweep_all = np.append(sweep_all, float(vote_threshold))
        L = len(self.engines)
        lab_it = iter(labels) if labels is not None else None
        lab_of: Dict[int, Any] = {}                 # lane -> the labels of the batch it was given last
        vote_of: Dict[int, Any] = {}                # lane -> ("device", labels per tile) / ("host", labels) of the fetch in flight
        tiles_of: Dict[int, Any] = {}               # lane -> the host tiles of the batch it was given last (band_stats: the host route reads them)
        band_of: Dict[int, Any] = {}                # lane -> ("device", labels per tile) / ("host", labels, tiles) of the histograms in flight
        if want_votes or sweep_all is not None:
            self.vote_fallbacks = 0
        if band_stats:
            self.band_fallbacks = 0

        def fetch_band(lane: int, n: int) -> None:
            eng = self.engines[lane]
            packed = eng._band_label_tables(n, lab_of[lane])
            if packed is None:
                self.band_fallbacks += 1
                band_of[lane] = ("host", lab_of[lane], tiles_of[lane])
            else:
                band_of[lane] = ("device", eng._band_enqueue(n, packed))

        def fetch(lane: int, n: int) -> None:
            eng = self.engines[lane]
            if not want_votes and sweep_all is None:
                self._fetch_async(eng, n)
                if band_stats:
                    fetch_band(lane, n)
                return
            packed = eng._vote_label_tables(n, lab_of[lane])
            if packed is None:
                self.vote_fallbacks += 1
                self._fetch_async(eng, n, masks=True)
                vote_of[lane] = ("host", lab_of[lane])
            elif poly_geo:
                self._fetch_async(eng, n)
                vote_of[lane] = ("device", (eng._pvote_enqueue(n, packed, sweep_all if sweep_all is not None else [vote_threshold]), lab_of[lane]))
            elif sweep_all is not None:
                self._fetch_async(eng, n)
                vote_of[lane] = ("device", eng._sweep_enqueue(n, packed, sweep_all))
            else:
                self._fetch_async(eng, n)
                vote_of[lane] = ("device", eng._vote_enqueue(n, packed, vote_threshold))
            if band_stats:
                fetch_band(lane, n)

        def with_band(lane: int, res: List[Instances]) -> List[Instances]:
            if not band_stats:
                return res
            what = band_of.pop(lane)
            if what[0] == "device":
                tables = self.engines[lane].band_hist_wait(len(res), what[1])
            else:
                from . import band_stats as band_mod
                tables = band_mod.band_hist_host(what[2], what[1])
            for inst, h in zip(res, tables):
                inst.band_hist = h
            return res

        def voted(lane: int, res: List[Instances]) -> List[Instances]:
            if not want_votes and sweep_all is None:
                return with_band(lane, res)
            from . import raster_vote
            kind, what = vote_of.pop(lane)
            if poly_geo:
                thr = sweep_all if sweep_all is not None else [vote_threshold]
                labs = what[1] if kind == "device" else what
                rows = self.engines[lane]._pvote_wait(len(res), what[0]) if kind == "device" else None
                if rows is None:                    # a flagged instance, or a batch that did not fit (already counted): the host route
                    self.vote_fallbacks += kind == "device"
                    rows = self.engines[lane].polygon_vote_host_rows(res, labs, thr)
                for inst, row in zip(res, rows):
                    if sweep_all is None:
                        inst.road_votes = raster_vote.sweep_slice(row, 0)
                        continue
                    if want_votes:
                        inst.road_votes = raster_vote.sweep_slice(row, sweep_T)
                    inst.road_vote_sweep = (row[0][:sweep_T], row[1][:sweep_T], row[2][:sweep_T], row[3])
                return with_band(lane, res)
            if sweep_all is not None:
                if kind == "device":
                    rows = self.engines[lane].road_votes_sweep_wait(len(res), False, what)
                else:
                    rows = raster_vote.vote_tables_host(res, what, self.engines[lane].spec.num_classes, thresholds=sweep_all)
                for inst, row in zip(res, rows):
                    if want_votes:                  # the appended slice is the vote at vote_threshold, bit for bit
                        inst.road_votes = raster_vote.sweep_slice(row, sweep_T)
                    inst.road_vote_sweep = (row[0][:sweep_T], row[1][:sweep_T], row[2][:sweep_T], row[3])
                return with_band(lane, res)
            if kind == "device":
                rows = self.engines[lane].road_votes_wait(len(res), False, what)
            else:
                rows = raster_vote.vote_tables_host(res, what, self.engines[lane].spec.num_classes, vote_threshold)
            for inst, row in zip(res, rows):
                inst.road_votes = row
            return with_band(lane, res)

        def counted(eng: Engine, res: List[Instances]) -> List[Instances]:
            # the lane's counts were published by its wait_results and stay until its next one: read them with the batch's results
            self.last_saturation = eng.saturation()
            return voted(self.engines.index(eng), res)
        inflight = []                               # (lane, n) of submitted batches not yet yielded
        T = self.timing = {"pull": 0.0, "wait_results": 0.0, "upload": 0.0, "enqueue": 0.0, "collect": 0.0, "batches": 0}
        clock = time.perf_counter
        it = iter(batches)
        while True:
            t0 = clock()
            tiles = next(it, None)                  # the source's time (decode wait) is not the pipeline's
            T["pull"] += clock() - t0
            if tiles is None:
                break
            T["batches"] += 1
            n = int(tiles.shape[0])
            lane = self.k % L
            e = self.engines[lane]
            self.k += 1
            if lab_it is not None:
                lab_of[lane] = next(lab_it)
            if band_stats:
                tiles_of[lane] = tiles
            if L == 1:                              # one lane has one set of host buffers: no look-ahead
                e.infer_device(e.upload_async(np.ascontiguousarray(tiles)), n)
                fetch(lane, n)
                yield counted(e, e.fetch_wait(n))
                continue
            done = None
            if len(inflight) == L:
                # this lane's previous batch: its result copy was enqueued one submit ago; once it has landed the lane's pinned
                # staging buffer (upload) is free again.  The other lane's batch keeps the GPU busy meanwhile.
                ol, on = inflight.pop(0)
                t0 = clock()
                self.engines[ol].wait_results()
                T["wait_results"] += clock() - t0
                done = (ol, on)
            t0 = clock()
            ptr = e.upload_async(np.ascontiguousarray(tiles))
            t1 = clock()
            T["upload"] += t1 - t0
            if not self.shared:
                e.infer_device(ptr, n)
                T["enqueue"] += clock() - t1
                res = None
                if done is not None:                # the lane's previous results leave its pinned buffers BEFORE the next copy into them is enqueued
                    t0 = clock()
                    res = counted(self.engines[done[0]], self.engines[done[0]].collect_results(done[1]))
                    T["collect"] += clock() - t0
                t1 = clock()
                fetch(lane, n)
                T["enqueue"] += clock() - t1
                inflight.append((lane, n))
                if res is not None:
                    yield res
                continue
            e.infer_phase(ptr, n, 0)
            if self._pending is not None:
                pl, pp, pn = self._pending
                self.engines[pl].infer_phase(pp, pn, 2)
                fetch(pl, pn)
                self._pending = None
            e.infer_phase(ptr, n, 1)
            T["enqueue"] += clock() - t1
            self._pending = (lane, ptr, n)
            inflight.append((lane, n))
            if done is not None:                    # host-side collection overlaps the batches just enqueued; this lane's next
                t0 = clock()
                res = counted(self.engines[done[0]], self.engines[done[0]].collect_results(done[1]))      # fetch_async comes one submit later
                T["collect"] += clock() - t0
                yield res
        if self._pending is not None:
            pl, pp, pn = self._pending
            self.engines[pl].infer_phase(pp, pn, 2)
            fetch(pl, pn)
            self._pending = None
        for ol, on in inflight:
            yield counted(self.engines[ol], self.engines[ol].fetch_wait(on))

    def sync(self) -> None:
        self.flush()
        for e in self.engines:
            e.sync()

    def close(self) -> None:
        for e in reversed(self.engines):     # lane 0 owns the shared stream: destroy it last
            e.close()


class Predictor:
    """Drop-in for ``detectron2.engine.DefaultPredictor``: ``predictor(im_bgr) -> {"instances": Instances}``.
    One two-lane pipeline is built per tile shape on first use (tilesets are single-shape: 256^2/512^2 z18 tiles,
    R:config/config_obj_detec.yaml:45).  ``predict_batch`` is the batched, streaming form the CLI shim uses.

    ``on_saturation``: what a batch whose activations were clamped to the fp16 range (precision fp16 / split) does --
    "warn" (default) issues one ``SaturationWarning`` per affected batch, "raise" raises ``RsSaturationError`` once the batch's results
    are collected, "ignore" does neither.  ``last_saturation`` holds, in every case, the non-zero counts by stage of the last result handed out:
    the image of ``__call__``, the whole ``predict_batch`` call (summed over its batches), the batch ``predict_stream`` yielded."""

    def __init__(self, spec: EngineSpec, weights: Dict[str, np.ndarray], max_batch: int = 16, device: int = 0, lanes: int = 2,
                 on_saturation: str = "warn", vectorize: str = "host", rdp_epsilon: float = 0.75):
        if on_saturation not in ("warn", "raise", "ignore"):
            raise ValueError(f"on_saturation must be 'warn', 'raise' or 'ignore', got {on_saturation!r}")
        if vectorize not in VECTORIZE_MODES:
            raise ValueError(f"vectorize must be one of {VECTORIZE_MODES}, got {vectorize!r}")
        # "device": the streaming forms (predict_batch, predict_stream) return Instances that carry polygons made on the GPU with
        # ``rdp_epsilon`` (<= 0: not simplified) and no masks; ``__call__`` always returns masks
        self.vectorize, self.rdp_epsilon = vectorize, float(rdp_epsilon)
        self.spec, self.weights, self.max_batch, self.device, self.lanes = spec, weights, max_batch, device, lanes
        self.on_saturation = on_saturation
        self.last_saturation: Dict[str, int] = {}
        self.vote_fallbacks = 0                     # batches of the last ``predict_stream(..., labels=...)`` that were voted on the host
        self.band_fallbacks = 0                     # batches of the last ``predict_stream(..., band_stats=True)`` counted on the host
        self._pipes: Dict[Tuple[int, int, int], LanePipeline] = {}

    def _saturated(self, sat: Dict[str, int], what: str) -> None:
        self.last_saturation = sat
        if not sat or self.on_saturation == "ignore":
            return
        msg = saturation_message(what, sat)
        if self.on_saturation == "raise":
            raise RsSaturationError(msg, sat)
        import warnings
        warnings.warn(msg, SaturationWarning, stacklevel=3)

    def _pipe(self, shape: Tuple[int, int, int]) -> LanePipeline:
        if shape not in self._pipes:
            self._pipes[shape] = LanePipeline(self.spec, self.weights, shape, self.max_batch, self.device, self.lanes,
                                              vectorize=self.vectorize, rdp_epsilon=self.rdp_epsilon)
        return self._pipes[shape]

    def prepare(self, shape: Tuple[int, int, int], warm: bool = True) -> None:
        """Build the lane pipeline for tiles of ``shape`` now instead of at the first batch, and (``warm``) run one blank tile through
        every lane so that the code objects are loaded and the per-kernel attributes set -- the CLI calls this while its decoder
        processes are still starting, the way the reference builds its ``DefaultPredictor`` before it loops over the tiles."""
        pipe = self._pipe(tuple(int(x) for x in shape))
        if warm:
            blank = np.zeros((1,) + tuple(int(x) for x in shape), np.uint8)
            for e in pipe.engines:
                e.infer(blank)

    def __call__(self, original_image: np.ndarray) -> Dict[str, Instances]:
        if original_image.ndim != 3:
            raise ValueError("expected an HWC image")
        eng = self._pipe(tuple(original_image.shape)).engines[0]
        out = {"instances": eng.infer(original_image[None])[0]}
        self._saturated(eng.saturation(), "image")
        return out

    def predict_batch(self, images: Sequence[np.ndarray]) -> List[Dict[str, Instances]]:
        """Any number of images; runs of equal shape are cut into batches of ``max_batch`` and streamed through the lanes
        (``LanePipeline.run``: uploads, forwards and result copies of consecutive batches overlap)."""
        out: List[Dict[str, Instances]] = []
        total: Dict[str, int] = {}                 # saturation counts of the whole call
        i = 0
        while i < len(images):
            shape = tuple(images[i].shape)
            j = i
            while j < len(images) and tuple(images[j].shape) == shape:
                j += 1
            chunks = (np.stack(images[k:min(k + self.max_batch, j)]) for k in range(i, j, self.max_batch))
            pipe = self._pipe(shape)
            for res in pipe.run(chunks):
                first = len(out)
                out.extend({"instances": r} for r in res)
                for k, v in pipe.last_saturation.items():
                    total[k] = total.get(k, 0) + v
                self._saturated(pipe.last_saturation, f"batch of images {first}..{len(out) - 1}")
            i = j
        self.last_saturation = total
        return out

    def predict_stream(self, batches, labels=None, vote_threshold: float = 0.0, band_stats: bool = False,
                       road_votes: bool = True, vote_sweep=None, vote_geometry: str = "pixels") -> "Iterator[List[Dict[str, Instances]]]":
        """Streaming form for a whole tileset: ``batches`` is an iterator of image lists (each at most ``max_batch`` images);
        yields one result list per batch, in order.  Consecutive batches of one tile shape flow through ONE
        ``LanePipeline.run`` generator, so the upload, forward and result copy of batch k+1 overlap batch k (calling
        ``predict_batch`` once per batch would drain the pipeline after every batch).  The iterator is pulled lazily, two
        batches ahead of what is yielded.  ``labels``: an iterable parallel to ``batches``, per batch the road labels of its tiles
        (``LanePipeline.run``); every yielded ``Instances`` then carries ``road_votes``, and ``vote_fallbacks`` counts the batches
        of the stream that were voted on the host.  Labels need batches of one tile shape.  ``band_stats=True``: every yielded
        ``Instances`` also carries ``band_hist`` (``LanePipeline.run``), ``band_fallbacks`` counts the batches whose histograms the
        host formed; ``road_votes=False`` leaves the vote out and the labels serve the histograms alone.  ``vote_sweep=thresholds``:
        every yielded ``Instances`` also carries ``road_vote_sweep``, the vote tables of every threshold (``LanePipeline.run``).
        ``vote_geometry="polygons"``: both on polygon areas (``LanePipeline.run``); needs ``vectorize="device"``, otherwise a
        ``ValueError`` before any forward."""
        from .raster_vote import check_vote_geometry
        check_vote_geometry(vote_geometry, self.vectorize)
        if band_stats and labels is None:
            raise ValueError("band_stats needs the road labels of every batch")
        if vote_sweep is not None and labels is None:
            raise ValueError("vote_sweep needs the road labels of every batch")
        it = iter(batches)
        lab_src = iter(labels) if labels is not None else None
        lab_q: List[Any] = []            # labels of the batches handed to the running pipeline and not yet taken by it
        carry: List[Any] = []            # a batch read ahead that does not fit the running pipeline (with its labels)
        k = 0                            # batches yielded
        self.vote_fallbacks = 0
        self.band_fallbacks = 0

        def next_batch():
            if carry:
                return carry.pop()
            b = next(it, None)
            return (None, None) if b is None else (b, next(lab_src) if lab_src is not None else None)

        def taken_labels():
            while True:
                yield lab_q.pop(0)

        while True:
            first, first_lab = next_batch()
            if first is None:
                return
            shapes = {tuple(im.shape) for im in first}
            if len(shapes) != 1 or len(first) > self.max_batch:
                if lab_src is not None:
                    raise ValueError("road labels need batches of one tile shape, at most max_batch tiles each")
                yield self.predict_batch(first)          # mixed shapes inside one batch: no streaming for it
                k += 1
                continue
            shape = shapes.pop()

            def run_of_shape(b=first, lab=first_lab):
                while b is not None:
                    if len(b) > self.max_batch or any(tuple(im.shape) != shape for im in b):
                        carry.append((b, lab))
                        return
                    lab_q.append(lab)
                    yield b if isinstance(b, np.ndarray) else np.stack(b)      # a decoded batch in shared memory is used in place
                    b, lab = next_batch()
            pipe = self._pipe(shape)
            before = pipe.vote_fallbacks if lab_src is None else 0
            band_before = 0
            for res in pipe.run(run_of_shape(), labels=taken_labels() if lab_src is not None else None, vote_threshold=vote_threshold,
                                band_stats=band_stats, road_votes=road_votes, vote_sweep=vote_sweep, vote_geometry=vote_geometry):
                self.vote_fallbacks += pipe.vote_fallbacks - before
                before = pipe.vote_fallbacks
                self.band_fallbacks += pipe.band_fallbacks - band_before
                band_before = pipe.band_fallbacks
                self._saturated(pipe.last_saturation, f"batch {k} of the stream")
                k += 1
                yield [{"instances": r} for r in res]

    def close(self) -> None:
        for p in self._pipes.values():
            p.close()
        self._pipes.clear()


MASK_TARGET_MODES = ("host", "device")
WGRAD_MODES = ("f32", "split")   # rs_trainer_set_wgrad_mode 0 / 1
DGRAD_MODES = ("f32", "split")   # rs_trainer_set_dgrad_mode 0 / 1
FWD_MODES = ("f32", "split")     # rs_trainer_set_fwd_mode 0 / 1
RS_EVAL_DOES_NOT_FIT = 2       # include/rs_engine.h: rs_engine_fetch_eval_async, the batch's ground truth exceeds the device pool
EVAL_GT_CAP = 128              # RS_EVAL_GT_CAP: ground truths per tile, and the row length of the count tables
VOTE_SWEEP_MAX = 32            # RS_VOTE_SWEEP_MAX: thresholds per vote sweep
RS_POLYGONS_DO_NOT_FIT = 1     # include/rs_engine.h: rs_trainer_set_polygons, the batch's polygons exceed the device pool
FREEZE_AT_VALUES = (0, 1, 2)   # MODEL.BACKBONE.FREEZE_AT a trainer implements (rs_train_options.freeze_at)


class RsTrainOptions(C.Structure):
    """include/rs_engine.h ``rs_train_options``."""
    _fields_ = [("struct_size", C.c_int32), ("freeze_at", C.c_int32)]


TRAIN_STATS_TABLE = 16         # csrc/train_stats.h TS_TABLE: int32 entries of the tensor "train_stats"
TRAIN_STATS_KEYS = ("rpn/num_pos_anchors", "rpn/num_neg_anchors", "roi_head/num_fg_samples", "roi_head/num_bg_samples",
                    "fast_rcnn/cls_accuracy", "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative",
                    "mask_rcnn/accuracy", "mask_rcnn/false_positive", "mask_rcnn/false_negative")


def train_stats_scalars(table: Sequence[int]) -> Dict[str, float]:
    """The integer table of ``rs_trainer_set_train_stats`` (include/rs_engine.h: [0..1] pos, neg anchors; [2..3] fg, bg sampled RoIs;
    [4..8] inst, correct, fgn, fg_correct, fg_as_bg; [9..13] pixels, incorrect, positive, false_pos, false_neg; [14] images) ->
    detectron2 0.6's training scalars under its names (``TRAIN_STATS_KEYS``), every ratio formed here in Python floats.  Omitted, as
    detectron2 omits them: the per-image means of a table without images, the three ``fast_rcnn/`` keys when no row counted, the two
    foreground ones when no foreground row did, the three ``mask_rcnn/`` keys when no mask pixel was counted (no entries, or MASK_ON
    false).  The values are those of ONE step: detectron2's 20-iteration median smoothing is not applied."""
    t = [int(v) for v in table]
    if len(t) != TRAIN_STATS_TABLE:
        raise ValueError(f"train_stats table of {len(t)} entries, expected {TRAIN_STATS_TABLE}")
    pos, neg, fg, bg, inst, correct, fgn, fg_correct, fg_as_bg, pixels, incorrect, positive, false_pos, false_neg, n = t[:15]
    out: Dict[str, float] = {}
    if n > 0:
        out["rpn/num_pos_anchors"] = pos / n
        out["rpn/num_neg_anchors"] = neg / n
        out["roi_head/num_fg_samples"] = fg / n
        out["roi_head/num_bg_samples"] = bg / n
    if inst > 0:
        out["fast_rcnn/cls_accuracy"] = correct / inst
        if fgn > 0:
            out["fast_rcnn/fg_cls_accuracy"] = fg_correct / fgn
            out["fast_rcnn/false_negative"] = fg_as_bg / fgn
    if pixels > 0:
        out["mask_rcnn/accuracy"] = 1.0 - incorrect / max(pixels, 1)
        out["mask_rcnn/false_positive"] = false_pos / max(pixels - positive, 1)
        out["mask_rcnn/false_negative"] = false_neg / max(positive, 1)
    return out


def _check_freeze_at(freeze_at: int) -> int:
    if isinstance(freeze_at, bool) or not isinstance(freeze_at, (int, np.integer)) or int(freeze_at) not in FREEZE_AT_VALUES:
        raise ValueError(f"MODEL.BACKBONE.FREEZE_AT (freeze_at) must be one of {FREEZE_AT_VALUES}, got {freeze_at!r}")
    return int(freeze_at)


def _check_wgrad(wgrad: str, spec: "EngineSpec") -> None:
    if wgrad not in WGRAD_MODES:
        raise ValueError(f"wgrad must be one of {WGRAD_MODES}, got {wgrad!r}")
    if wgrad == "split" and spec.precision == "fp16":
        raise ValueError("wgrad='split' serves the fp32 trainer (precision='fp32'); the fp16 trainer already runs on the fp16 matrix cores")


def _check_dgrad(dgrad: str, spec: "EngineSpec") -> None:
    if dgrad not in DGRAD_MODES:
        raise ValueError(f"dgrad must be one of {DGRAD_MODES}, got {dgrad!r}")
    if dgrad == "split" and spec.precision == "fp16":
        raise ValueError("dgrad='split' serves the fp32 trainer (precision='fp32'); the fp16 trainer already runs on the fp16 matrix cores")


def _check_fwd(fwd: str, spec: "EngineSpec") -> None:
    if fwd not in FWD_MODES:
        raise ValueError(f"fwd must be one of {FWD_MODES}, got {fwd!r}")
    if fwd == "split" and spec.precision == "fp16":
        raise ValueError("fwd='split' serves the fp32 trainer (precision='fp32'); the fp16 trainer already runs on the fp16 matrix cores")


class Trainer:
    """Training engine (include/rs_engine.h ``rs_trainer_*``): forward engine + flat fp32
    master / gradient / momentum buffers + backward stage list.  ``train_step`` = ``SimpleTrainer.run_step`` up to
    ``losses.backward()`` (forward, label assignment + sampling, the five losses, backward of every trainable layer);
    ``apply_sgd`` = the optimiser step; ``allreduce_gradients`` = DDP's gradient averaging over RCCL."""

    def __init__(self, spec: EngineSpec, weights: Dict[str, np.ndarray], tile_shape: Tuple[int, int, int], batch: int = 2,
                 device: int = 0, loss_scale: float = 1.0, lib_path: Optional[str] = None, mask_targets: str = "host", wgrad: str = "f32",
                 dgrad: str = "f32", fwd: str = "f32", train_stats: bool = False, freeze_at: int = 2, solver: Optional[SolverOptions] = None):
        """``solver``: a ``SolverOptions`` -- gradient clipping, Nesterov momentum and the bias parameter groups of the optimiser step
        (``set_solver``).  ``None`` (default): ``apply_sgd`` is plain SGD with momentum over the whole flat buffer, as it always was.

        ``freeze_at``: detectron2's ``MODEL.BACKBONE.FREEZE_AT``, fixed at creation because it changes the graph.  2 (default): the
        stem and res2 are frozen.  1: res2 is trained too.  0: the stem convolution as well -- what a detector with a fourth input band
        needs, whose stem channel no public checkpoint holds.  The forward engine then runs res2 (and at 0 the stem) unfused, the
        backward goes on below res3, and the flat buffers gain the groups "res2" and "stem" (``buckets()``).

        ``train_stats``: count detectron2's training diagnostics (anchor and RoI sample counts, the box head's classification
        accuracies, the mask head's pixel accuracies) on the GPU behind the loss stages of every step; ``train_stats()`` returns them
        under detectron2's names.  Off by default; losses and gradients are the same bits either way.  ``set_train_stats`` switches
        between steps.

        ``fwd``: the forward product Y = X * W of the fp32 trainer's convolution and linear stages, with the same two values: "split"
        runs it on the fp16 matrix cores from hi + lo fp16 planes of X and of the folded weight; activations stay fp32,
        the stem and the mask deconvolution keep their fp32 kernels, and validation inference through ``inference_engine`` follows the
        mode.  ``set_fwd_mode`` switches between steps.

        ``dgrad``: the input-gradient product dX = dY * W^T of the fp32 trainer's convolution and linear stages, with the same two
        values: "split" runs it on the fp16 matrix cores from hi + lo fp16 planes; the mask deconvolution and RoIAlign
        backward stay fp32.  ``set_dgrad_mode`` switches between steps.

        ``wgrad``: the weight-gradient product of the fp32 trainer.  "f32" (default): fp32 matrix cores.  "split": the fp32 operands
        become hi + lo fp16 planes and the product runs on the fp16 matrix cores; storage, forward and input gradients
        stay fp32.  ``set_wgrad_mode`` switches between steps.

        ``mask_targets``: where ``train_step`` rasterises the mask head's ground-truth crops.  "host" (default): read the sampled
        RoIs back, rasterise on host threads, upload (``mask_entries`` + ``mask_backward``).  "device": upload the batch's polygons
        with the targets and rasterise on the GPU (``set_polygons`` + ``mask_backward_device``) -- the same bytes, no host wait
        inside the step; a batch whose polygons do not fit the device pool runs the host path for that step
        (``mask_target_fallbacks`` counts them)."""
        if mask_targets not in MASK_TARGET_MODES:
            raise ValueError(f"mask_targets must be one of {MASK_TARGET_MODES}, got {mask_targets!r}")
        _check_wgrad(wgrad, spec)
        _check_dgrad(dgrad, spec)
        _check_fwd(fwd, spec)
        self.freeze_at = _check_freeze_at(freeze_at)
        self.mask_targets = mask_targets
        self.mask_target_fallbacks = 0
        self.lib = lib = load_library(lib_path)
        vp, i32 = C.c_void_p, C.c_int
        lib.rs_trainer_create.argtypes = [C.POINTER(RsSpec), vp, C.c_size_t, i32, i32, i32, i32, i32, C.c_float, C.POINTER(vp)]
        lib.rs_trainer_create2.argtypes = [C.POINTER(RsSpec), vp, C.c_size_t, i32, i32, i32, i32, i32, C.c_float, C.POINTER(RsTrainOptions), C.POINTER(vp)]
        lib.rs_trainer_destroy.argtypes = [vp]
        lib.rs_trainer_destroy.restype = None
        lib.rs_trainer_engine.argtypes = [vp]
        lib.rs_trainer_engine.restype = vp
        lib.rs_trainer_forward_trunk.argtypes = [vp, vp, i32]
        lib.rs_trainer_backward_trunk.argtypes = [vp, i32]
        lib.rs_trainer_apply_sgd.argtypes = [vp, C.c_float, C.c_float, C.c_float]
        lib.rs_trainer_set_targets.argtypes = [vp, vp, vp, vp, i32, i32]
        lib.rs_trainer_set_image_sizes.argtypes = [vp, vp, vp, i32]
        lib.rs_trainer_rpn_step.argtypes = [vp, i32, C.c_uint32, i32]
        lib.rs_trainer_rpn_forward.argtypes = [vp, i32]
        lib.rs_trainer_rpn_targets_async.argtypes = [vp, i32, C.c_uint32]
        lib.rs_trainer_roi_step.argtypes = [vp, i32, C.c_uint32]
        lib.rs_trainer_set_sampling.argtypes = [vp, i32, C.c_float, i32, C.c_float]
        lib.rs_trainer_set_rpn_topk.argtypes = [vp, i32, i32]
        lib.rs_trainer_set_wgrad_mode.argtypes = [vp, i32]
        if hasattr(lib, "rs_trainer_set_dgrad_mode"):
            lib.rs_trainer_set_dgrad_mode.argtypes = [vp, i32]
        if hasattr(lib, "rs_trainer_set_fwd_mode"):
            lib.rs_trainer_set_fwd_mode.argtypes = [vp, i32]
        lib.rs_trainer_set_grad_divisor.argtypes = [vp, C.c_float]
        lib.rs_trainer_copy_state.argtypes = [vp, vp]
        lib.rs_trainer_grad_buffer.argtypes = [vp]
        lib.rs_trainer_set_loss_scale.argtypes = [vp, C.c_float]
        lib.rs_trainer_fetch_rois.argtypes = [vp, C.c_int, vp, vp, vp]
        lib.rs_trainer_grad_buffer.restype = vp
        lib.rs_trainer_master_buffer.argtypes = [vp]
        lib.rs_trainer_master_buffer.restype = vp
        lib.rs_trainer_bucket_count.argtypes = [vp]
        lib.rs_trainer_bucket_info.argtypes = [vp, i32, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.rs_trainer_bucket_wait.argtypes = [vp, i32, vp]
        lib.rs_trainer_bucket_sync.argtypes = [vp, i32]
        lib.rs_trainer_wait_stream.argtypes = [vp, vp]
        lib.rs_trainer_mask_forward.argtypes = [vp, i32]
        lib.rs_trainer_mask_backward.argtypes = [vp, i32, vp, i32]
        lib.rs_trainer_set_polygons.argtypes = [vp, vp, vp, vp, vp, vp, i32]
        lib.rs_trainer_mask_backward_device.argtypes = [vp, i32]
        lib.rs_trainer_sync.argtypes = [vp]
        lib.rs_trainer_set_profiling.argtypes = [vp, i32]
        lib.rs_trainer_stage_count.argtypes = [vp]
        lib.rs_trainer_stage_info.argtypes = [vp, i32, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        lib.rs_trainer_tensor.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.rs_trainer_tensor_count.argtypes = [vp]
        lib.rs_trainer_tensor_name.argtypes = [vp, i32, C.c_char_p]
        lib.rs_trainer_param_count.argtypes = [vp]
        lib.rs_trainer_param_count.restype = C.c_int64
        self.spec = spec
        self.tile_h, self.tile_w, self.tile_c = (int(x) for x in tile_shape)
        self.batch = int(batch)
        blob = pack_weights(spec, weights, train=True, freeze_at=self.freeze_at)
        rs = make_rs_spec(spec)
        h = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        opts = RsTrainOptions(C.sizeof(RsTrainOptions), self.freeze_at)
        _check(lib, lib.rs_trainer_create2(C.byref(rs), buf, len(blob), device, self.batch, self.tile_h, self.tile_w, self.tile_c,
                                           float(loss_scale), C.byref(opts), C.byref(h)), "rs_trainer_create2")
        self._h = h
        self._eng = C.c_void_p(lib.rs_trainer_engine(h))
        self.wgrad = "f32"
        if wgrad != "f32":
            self.set_wgrad_mode(wgrad)
        self.dgrad = "f32"
        if dgrad != "f32":
            self.set_dgrad_mode(dgrad)
        self.fwd = "f32"
        if fwd != "f32":
            self.set_fwd_mode(fwd)
        self.train_stats_on = False
        if train_stats:
            self.set_train_stats(True)
        self.solver: Optional[SolverOptions] = None
        if solver is not None:
            self.set_solver(solver)

    def _tensor_ptr(self, name: str, engine: bool = False):
        p, dt, nd, halo = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        dims = (C.c_int64 * 5)()
        if engine:
            _check(self.lib, self.lib.rs_engine_tensor(self._eng, name.encode(), C.byref(p), C.byref(dt), C.byref(nd), dims, C.byref(halo)), f"tensor {name}")
        else:
            _check(self.lib, self.lib.rs_trainer_tensor(self._h, name.encode(), C.byref(p), C.byref(dt), C.byref(nd), dims, C.byref(halo)), f"tensor {name}")
        return int(p.value), np.dtype(DT_NP[dt.value]), tuple(int(dims[i]) for i in range(nd.value)), halo.value

    def tensor(self, name: str, engine: bool = False, strip_halo: bool = True) -> np.ndarray:
        """Copy a trainer tensor ("d:<act>", "g:<layer>.w", "m:<layer>.w") or, with ``engine=True``, a forward tensor to the host."""
        ptr, dt, shape, halo = self._tensor_ptr(name, engine)
        a = np.empty(shape, dt)
        self.sync()                     # the trainer's stream is non-blocking: a plain memcpy would not wait for it
        _check(self.lib, self.lib.rs_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes), "rs_memcpy_d2h")
        if strip_halo and halo:
            a = a[:, halo:-halo, halo:-halo]
        return a

    def set_tensor(self, name: str, interior: np.ndarray) -> None:
        """Write the interior of an activation-gradient tensor (the halo stays zero)."""
        ptr, dt, shape, halo = self._tensor_ptr(name)
        full = np.zeros(shape, dt)
        n = interior.shape[0]
        if halo:
            full[:n, halo:-halo, halo:-halo] = interior.astype(dt)
        else:
            full[:n] = interior.astype(dt)
        _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(ptr), full.ctypes.data_as(C.c_void_p), full.nbytes), "rs_memcpy_h2d")

    def tensor_names(self) -> List[str]:
        buf = C.create_string_buffer(96)
        out = []
        for i in range(self.lib.rs_trainer_tensor_count(self._h)):
            self.lib.rs_trainer_tensor_name(self._h, i, buf)
            out.append(buf.value.decode())
        return out

    def upload_tiles(self, tiles: np.ndarray) -> int:
        tiles = np.ascontiguousarray(tiles)
        assert tiles.dtype == np.uint8 and tiles.shape[1:] == (self.tile_h, self.tile_w, self.tile_c) and tiles.shape[0] <= self.batch
        ptr, _, _, _ = self._tensor_ptr("tiles", engine=True)
        _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(ptr), tiles.ctypes.data_as(C.c_void_p), tiles.nbytes), "rs_memcpy_h2d")
        return ptr

    def forward_trunk(self, tiles_ptr: int, n: int) -> None:
        _check(self.lib, self.lib.rs_trainer_forward_trunk(self._h, C.c_void_p(tiles_ptr), n), "rs_trainer_forward_trunk")

    def set_targets(self, gt_boxes: Sequence[np.ndarray], gt_classes: Sequence[np.ndarray]) -> None:
        """Ground truth per image: boxes (k_i, 4) in NETWORK-INPUT pixels, classes (k_i,)."""
        n = len(gt_boxes)
        cap = max(1, max(int(b.shape[0]) for b in gt_boxes))
        bx = np.zeros((n, cap, 4), np.float32)
        cl = np.zeros((n, cap), np.int32)
        cnt = np.zeros(n, np.int32)
        for i, (b, c) in enumerate(zip(gt_boxes, gt_classes)):
            k = int(b.shape[0])
            bx[i, :k], cl[i, :k], cnt[i] = b, c, k
        _check(self.lib, self.lib.rs_trainer_set_targets(self._h, bx.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p),
                                                         cnt.ctypes.data_as(C.c_void_p), n, cap), "rs_trainer_set_targets")

    def set_image_sizes(self, sizes: Optional[Sequence[int]]) -> List[Tuple[int, int]]:
        """``INPUT.MIN_SIZE_TRAIN`` drawn PER IMAGE (R:config/detectron2_config_3bands.yaml:31-38; [EXT d2: DatasetMapper ->
        ResizeShortestEdge per record, ImageList.from_tensors pads the batch to its largest image]): image i of the coming
        batches is resized to shortest edge ``sizes[i]`` inside this trainer's canvas (whose own size must be the largest of the
        batch), zeros beyond it, proposals clipped to it.  ``None`` / empty: one size for all again.  Returns the (h, w) per
        image -- ground truth of image i is in THOSE pixels."""
        from .spec import resize_shortest_edge_shape
        if not sizes:
            _check(self.lib, self.lib.rs_trainer_set_image_sizes(self._h, None, None, 0), "rs_trainer_set_image_sizes")
            self._image_sizes = None
            return []
        hw = [resize_shortest_edge_shape(self.tile_h, self.tile_w, int(s), self.spec.max_size_test) for s in sizes]
        if list(sizes) == getattr(self, "_image_sizes", None):
            return hw
        nh = np.asarray([h for h, _ in hw], np.int32)
        nw = np.asarray([w for _, w in hw], np.int32)
        _check(self.lib, self.lib.rs_trainer_set_image_sizes(self._h, nh.ctypes.data_as(C.c_void_p), nw.ctypes.data_as(C.c_void_p), len(hw)),
               "rs_trainer_set_image_sizes")
        self._image_sizes = list(sizes)
        return hw

    def rpn_step(self, n: int, seed: int = 1, external_labels: bool = False) -> None:
        _check(self.lib, self.lib.rs_trainer_rpn_step(self._h, n, seed & 0xFFFFFFFF, int(external_labels)), "rs_trainer_rpn_step")

    def rpn_forward(self, n: int) -> None:
        _check(self.lib, self.lib.rs_trainer_rpn_forward(self._h, n), "rs_trainer_rpn_forward")

    def roi_step(self, n: int, seed: int = 1) -> None:
        _check(self.lib, self.lib.rs_trainer_roi_step(self._h, n, seed & 0xFFFFFFFF), "rs_trainer_roi_step")

    def mask_forward(self, n: int) -> None:
        _check(self.lib, self.lib.rs_trainer_mask_forward(self._h, n), "rs_trainer_mask_forward")

    def mask_backward(self, n: int, targets: np.ndarray) -> None:
        """targets: (n_entries, 28, 28) bool/uint8 gt masks of the mask-head entries, in entry order."""
        t = np.ascontiguousarray(targets.astype(np.uint8))
        _check(self.lib, self.lib.rs_trainer_mask_backward(self._h, n, t.ctypes.data_as(C.c_void_p) if t.size else None, int(t.shape[0])),
               "rs_trainer_mask_backward")

    def set_polygons(self, gt_polygons: Sequence[Sequence[Sequence[np.ndarray]]]) -> bool:
        """Device mask targets: upload the batch's ground-truth polygons (gt_polygons[image][gt index] = list of polygons, network-input
        pixels, as ``mask_entries`` takes them).  Call after ``set_targets``.  False: they do not fit the device pool (include/rs_engine.h
        ``rs_trainer_set_polygons``) and nothing was uploaded -- run this step through ``mask_entries`` + ``mask_backward``."""
        n = len(gt_polygons)
        arrs = [np.asarray(p, np.float64).reshape(-1) for img in gt_polygons for polys in img for p in polys]
        lens = np.array([a.size for a in arrs], np.int32)
        off = np.zeros(max(len(arrs), 1), np.int64)
        if len(arrs) > 1:
            off[1:] = np.cumsum(lens[:-1], dtype=np.int64)
        flat = np.ascontiguousarray(np.concatenate(arrs)) if arrs else np.zeros(1)
        inst_first = np.zeros(sum(len(img) for img in gt_polygons) + 1, np.int32)
        inst_first[1:] = np.cumsum([len(polys) for img in gt_polygons for polys in img])
        image_first = np.zeros(n + 1, np.int32)
        image_first[1:] = np.cumsum([len(img) for img in gt_polygons])
        lens = np.ascontiguousarray(lens) if lens.size else np.zeros(1, np.int32)
        rc = self.lib.rs_trainer_set_polygons(self._h, flat.ctypes.data, off.ctypes.data, lens.ctypes.data, inst_first.ctypes.data,
                                              image_first.ctypes.data, n)
        if rc == RS_POLYGONS_DO_NOT_FIT:
            return False
        _check(self.lib, rc, "rs_trainer_set_polygons")
        return True

    def mask_backward_device(self, n: int) -> None:
        """``mask_backward`` with the targets rasterised on the GPU from the polygons of ``set_polygons`` (tensor "mask_targets")."""
        _check(self.lib, self.lib.rs_trainer_mask_backward_device(self._h, n), "rs_trainer_mask_backward_device")

    def mask_entries(self, gt_polygons: Sequence[Sequence[Sequence[np.ndarray]]], n: int) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
        """Host part of the mask branch: gt masks of the sampled foreground RoIs (``PolygonMasks.crop_and_resize``).
        gt_polygons[image][gt index] = list of polygons ([x0,y0,...], network-input pixels).  Returns (targets, [(image, slot)])."""
        from .train_targets import rasterize_entries
        boxes = np.empty((n, 1024, 4), np.float32)
        gti = np.empty((n, 1024), np.int32)
        cnt = np.empty((n, 2), np.int32)
        _check(self.lib, self.lib.rs_trainer_fetch_rois(self._h, n, boxes.ctypes.data_as(C.c_void_p), gti.ctypes.data_as(C.c_void_p),
                                                        cnt.ctypes.data_as(C.c_void_p)), "rs_trainer_fetch_rois")
        side = 2 * self.spec.mask_pooler_resolution
        first = np.zeros(n + 1, np.int64)                      # instance index of image i's gt j = first[i] + j
        first[1:] = np.cumsum([len(gt_polygons[i]) for i in range(n)])
        instances = [polys for i in range(n) for polys in gt_polygons[i]]
        where = [(i, j) for i in range(n) for j in range(min(int(cnt[i, 0]), 256))]
        if not where:
            return np.zeros((0, side, side), bool), where
        ii = np.array([w[0] for w in where]); jj = np.array([w[1] for w in where])
        return rasterize_entries(instances, first[ii] + gti[ii, jj], boxes[ii, jj], side), where

    # ------------------------------------------------------------------ a whole step
    def train_step(self, tiles: np.ndarray, gt_boxes: Sequence[np.ndarray], gt_classes: Sequence[np.ndarray],
                   gt_polygons: Optional[Sequence[Sequence[Sequence[np.ndarray]]]], seed: int, allreduce: bool = False,
                   sizes: Optional[Sequence[int]] = None) -> Dict[str, float]:
        """Forward + losses + backward of one batch (``SimpleTrainer.run_step`` up to ``losses.backward()``): gradients end
        up in the flat gradient buffer; returns the five losses.  ``gt_*`` in NETWORK-INPUT pixels.  ``allreduce``: enqueue
        the data-parallel gradient all-reduce (``allreduce_gradients``) behind the backward pass before the losses are read
        back, so that the collectives of the early buckets overlap the rest of the backward.  ``sizes``: shortest-edge size
        per image (``set_image_sizes``); ``None`` keeps whatever was set last."""
        n = int(tiles.shape[0])
        if sizes is not None:
            self.set_image_sizes(sizes if any(int(s) != self.spec.min_size_test for s in sizes) else None)
        self.set_targets(gt_boxes, gt_classes)
        on_device = False
        if self.spec.mask_on and self.mask_targets == "device":
            on_device = self.set_polygons(gt_polygons[:n])
            if not on_device:
                self.mask_target_fallbacks += 1          # this step alone takes the host path; nothing is truncated
        # the RPN's targets depend on the ground truth and the seed only: on the side stream, ahead of the forward pass
        _check(self.lib, self.lib.rs_trainer_rpn_targets_async(self._h, n, seed & 0xFFFFFFFF), "rs_trainer_rpn_targets_async")
        self.forward_trunk(self.upload_tiles(tiles), n)
        self.rpn_forward(n)
        self.roi_step(n, seed)
        if self.spec.mask_on:
            self.mask_forward(n)
            if on_device:
                self.mask_backward_device(n)
            else:
                targets, _ = self.mask_entries(gt_polygons, n)
                self.mask_backward(n, targets)
        self.rpn_step(n, seed)
        self.backward_trunk(n)
        if allreduce:
            self.allreduce_gradients()
        l = self.tensor("losses")
        names = ("loss_rpn_cls", "loss_rpn_loc", "loss_cls", "loss_box_reg", "loss_mask")
        return {k: float(l[i]) for i, k in enumerate(names)}

    def copy_state_from(self, other: "Trainer") -> None:
        """Carry master weights + momentum over from ``other`` (a trainer of another input size) and refold."""
        _check(self.lib, self.lib.rs_trainer_copy_state(self._h, other._h), "rs_trainer_copy_state")
        self.dgrad = other.dgrad                 # rs_trainer_copy_state carries the input-gradient mode
        self.fwd = other.fwd                     # ... and the forward mode
        self.solver = other.solver               # ... and the solver

    def inference_engine(self) -> Engine:
        """The trainer's forward engine as an inference ``Engine`` (same device buffers, current weights): validation detections
        without a second copy of the network.  Valid until the trainer is closed; do not interleave with a training step."""
        if getattr(self, "_infer", None) is None:
            self._infer = Engine.from_handle(self.lib, int(self._eng.value), self.spec, (self.tile_h, self.tile_w, self.tile_c), self.batch)
        return self._infer

    def set_profiling(self, on: bool) -> None:
        """HIP events around every stage of the following training steps (``stage_times`` reads them)."""
        _check(self.lib, self.lib.rs_trainer_set_profiling(self._h, 1 if on else 0), "rs_trainer_set_profiling")

    def stage_times(self) -> List[Dict[str, Any]]:
        """Per stage of the training step since ``set_profiling(True)``: name, ms_total, calls, algorithmic flops of one execution,
        side (True: runs on the weight-gradient side stream, next to the chain)."""
        out = []
        name = C.create_string_buffer(96)
        ms, fl, calls, sd = C.c_double(), C.c_double(), C.c_int32(), C.c_int32()
        for i in range(self.lib.rs_trainer_stage_count(self._h)):
            _check(self.lib, self.lib.rs_trainer_stage_info(self._h, i, name, C.byref(ms), C.byref(calls), C.byref(fl), C.byref(sd)), "rs_trainer_stage_info")
            out.append({"name": name.value.decode(), "ms_total": ms.value, "calls": calls.value, "flops": fl.value, "side": bool(sd.value)})
        return out

    def buckets(self) -> List[Tuple[str, int, int]]:
        """Gradient buckets (name, offset, count in floats of the flat gradient buffer) in the order a step completes them."""
        out = []
        name = C.create_string_buffer(96)
        off, cnt = C.c_int64(), C.c_int64()
        for i in range(self.lib.rs_trainer_bucket_count(self._h)):
            _check(self.lib, self.lib.rs_trainer_bucket_info(self._h, i, name, C.byref(off), C.byref(cnt)), "rs_trainer_bucket_info")
            out.append((name.value.decode(), int(off.value), int(cnt.value)))
        return out

    def flat(self, which: str = "grad") -> np.ndarray:
        """Host copy of the whole flat fp32 gradient ("grad") or master-weight ("master") buffer (waits for the step)."""
        ptr = int(self.lib.rs_trainer_grad_buffer(self._h) if which == "grad" else self.lib.rs_trainer_master_buffer(self._h))
        a = np.empty(self.param_count, np.float32)
        self.sync()
        _check(self.lib, self.lib.rs_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), a.nbytes), "rs_memcpy_d2h")
        return a

    def write_flat_grad(self, g: np.ndarray) -> None:
        g = np.ascontiguousarray(g, np.float32)
        assert g.shape == (self.param_count,)
        self.sync()
        _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(int(self.lib.rs_trainer_grad_buffer(self._h))), g.ctypes.data_as(C.c_void_p), g.nbytes), "rs_memcpy_h2d")

    def allreduce_gradients(self, force: bool = False) -> None:
        """DistributedDataParallel's gradient averaging: SUM every gradient bucket over the ranks of the default process group
        and set the divisor the SGD step applies.  Buckets are reduced in the order the step completes them (heads, FPN,
        res5, res4, res3 -- ``buckets()``), each behind its own completion events:

        * RCCL (backend "nccl"): the bucket is handed to torch.distributed in place (``__cuda_array_interface__`` view of the
          device buffer) as an ASYNCHRONOUS all-reduce; torch's current stream is first made to wait (device side) for the
          bucket's events, so the call returns at once and the collective runs over xGMI while the trainer's streams are still
          computing the later buckets' gradients.  Afterwards the trainer's stream waits for the collectives (one event).
          One process per GPU; the host never blocks here.
        * gloo (CPU tests, several ranks on one card): per bucket, wait for its events on the host, reduce through a host copy.

        Call it after the backward pass has been ENQUEUED (``train_step(..., allreduce=True)`` does, before it reads the
        losses back) and before ``apply_sgd``."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not force):
            return                      # ``force``: run the collectives even in a one-rank group (exercises the RCCL path on one GPU)
        ptr = int(self.lib.rs_trainer_grad_buffer(self._h))
        if dist.get_backend() == "nccl":
            cur = torch.cuda.current_stream()
            works = []
            for i, (_, off, cnt) in enumerate(self.buckets()):
                _check(self.lib, self.lib.rs_trainer_bucket_wait(self._h, i, C.c_void_p(cur.cuda_stream)), "rs_trainer_bucket_wait")

                class _Buf:                      # zero-copy view of the bucket inside the device buffer
                    __cuda_array_interface__ = {"shape": (cnt,), "typestr": "<f4", "data": (ptr + 4 * off, False), "version": 2}
                t = torch.as_tensor(_Buf(), device="cuda")
                works.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True))
            for w in works:
                w.wait()                         # torch's current stream waits for the collective (no host block)
            _check(self.lib, self.lib.rs_trainer_wait_stream(self._h, C.c_void_p(cur.cuda_stream)), "rs_trainer_wait_stream")
        else:
            for i, (_, off, cnt) in enumerate(self.buckets()):
                _check(self.lib, self.lib.rs_trainer_bucket_sync(self._h, i), "rs_trainer_bucket_sync")
                host = np.empty(cnt, np.float32)
                _check(self.lib, self.lib.rs_memcpy_d2h(host.ctypes.data_as(C.c_void_p), C.c_void_p(ptr + 4 * off), host.nbytes), "rs_memcpy_d2h")
                t = torch.from_numpy(host)
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
                _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(ptr + 4 * off), host.ctypes.data_as(C.c_void_p), host.nbytes), "rs_memcpy_h2d")
        _check(self.lib, self.lib.rs_trainer_set_grad_divisor(self._h, float(dist.get_world_size())), "rs_trainer_set_grad_divisor")

    def export_weights(self, base: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
        """Current weights under detectron2's checkpoint key names: ``base`` (the weights the trainer was created from) with
        every trainable tensor replaced by its fp32 master copy, converted back from the engine's GEMM layouts."""
        from .weights import master_to_d2
        return master_to_d2(self.spec, base, lambda name: self.tensor(name), freeze_at=self.freeze_at)

    def set_wgrad_mode(self, mode: str) -> None:
        """Weight-gradient product of the following steps: one of ``WGRAD_MODES``.  An fp16 trainer refuses "split" (``RsError``)."""
        if mode not in WGRAD_MODES:
            raise ValueError(f"wgrad must be one of {WGRAD_MODES}, got {mode!r}")
        _check(self.lib, self.lib.rs_trainer_set_wgrad_mode(self._h, WGRAD_MODES.index(mode)), "rs_trainer_set_wgrad_mode")
        self.wgrad = mode

    def set_dgrad_mode(self, mode: str) -> None:
        """Input-gradient product of the following steps: one of ``DGRAD_MODES``.  An fp16 trainer refuses "split" (``RsError``)."""
        if mode not in DGRAD_MODES:
            raise ValueError(f"dgrad must be one of {DGRAD_MODES}, got {mode!r}")
        _check(self.lib, self.lib.rs_trainer_set_dgrad_mode(self._h, DGRAD_MODES.index(mode)), "rs_trainer_set_dgrad_mode")
        self.dgrad = mode

    def set_fwd_mode(self, mode: str) -> None:
        """Forward product of the following steps (and of validation inference on this trainer's engine): one of ``FWD_MODES``.  An
        fp16 trainer refuses "split" (``RsError``)."""
        if mode not in FWD_MODES:
            raise ValueError(f"fwd must be one of {FWD_MODES}, got {mode!r}")
        _check(self.lib, self.lib.rs_trainer_set_fwd_mode(self._h, FWD_MODES.index(mode)), "rs_trainer_set_fwd_mode")
        self.fwd = mode

    def set_train_stats(self, on: bool) -> None:
        """Training diagnostics of the following steps on (counted on the GPU, ``train_stats()`` reads them) or off."""
        if not hasattr(self.lib, "rs_trainer_set_train_stats"):
            raise RsError("this librs_engine.so has no rs_trainer_set_train_stats (an older build)")
        _check(self.lib, self.lib.rs_trainer_set_train_stats(self._h, 1 if on else 0), "rs_trainer_set_train_stats")
        self.train_stats_on = bool(on)

    def set_solver(self, solver: SolverOptions) -> None:
        """The solver of the following ``apply_sgd`` calls (include/rs_engine.h ``rs_trainer_set_solver``): clipping, Nesterov, bias groups.
        The first call adds the tensors "grad_norms" and "clip_coef" to ``tensor_names()``."""
        if not hasattr(self.lib, "rs_trainer_set_solver"):
            raise RsError("this librs_engine.so has no rs_trainer_set_solver (an older build)")
        if not isinstance(solver, SolverOptions):
            raise TypeError(f"solver must be a SolverOptions, got {type(solver).__name__}")
        st = solver.to_struct()
        _check(self.lib, self.lib.rs_trainer_set_solver(self._h, C.byref(st)), "rs_trainer_set_solver")
        self.solver = solver

    def segments(self) -> List[Tuple[str, int, int, bool]]:
        """The trainable tensors in buffer order: (name "<layer>.w" / "<layer>.b", offset, count in floats of the flat buffers, is_bias)."""
        out = []
        name = C.create_string_buffer(96)
        off, cnt, bias = C.c_int64(), C.c_int64(), C.c_int32()
        for i in range(self.lib.rs_trainer_segment_count(self._h)):
            _check(self.lib, self.lib.rs_trainer_segment_info(self._h, i, name, C.byref(off), C.byref(cnt), C.byref(bias)), "rs_trainer_segment_info")
            out.append((name.value.decode(), int(off.value), int(cnt.value), bool(bias.value)))
        return out

    def grad_norms(self) -> Dict[str, float]:
        """Name -> gradient norm of every trainable tensor as the last ``apply_sgd`` measured it (unscaled, rank-averaged gradient; the
        solver's NORM_TYPE).  Only a solver that clips by "norm" or "full_model" measures norms.  One small copy and a wait for the
        trainer's stream: for diagnosis, not for every step."""
        if self.solver is None or self.solver.clip_type not in ("norm", "full_model"):
            raise RsError("gradient norms are measured by a solver with clip_type 'norm' or 'full_model' (set_solver)")
        norms = self.tensor("grad_norms")
        return {s[0]: float(norms[i]) for i, s in enumerate(self.segments())}

    def train_stats_table(self) -> np.ndarray:
        """The int32 [16] table of the last step (include/rs_engine.h ``rs_trainer_set_train_stats``); synchronises the trainer's stream."""
        if not self.train_stats_on:
            raise RsError("training diagnostics are off: Trainer(..., train_stats=True) or set_train_stats(True) before the step")
        return self.tensor("train_stats")

    def train_stats(self) -> Dict[str, float]:
        """detectron2's training scalars of the last step (``train_stats_scalars`` of the table): 64 bytes cross PCIe."""
        return train_stats_scalars(self.train_stats_table())

    def set_sampling(self, rpn_batch: int = 256, rpn_positive_fraction: float = 0.5, roi_batch: int = 1024, roi_positive_fraction: float = 0.25) -> None:
        _check(self.lib, self.lib.rs_trainer_set_sampling(self._h, rpn_batch, rpn_positive_fraction, roi_batch, roi_positive_fraction), "rs_trainer_set_sampling")

    def set_rpn_topk(self, pre_nms_topk_train: int = 2000, post_nms_topk_train: int = 1000) -> None:
        _check(self.lib, self.lib.rs_trainer_set_rpn_topk(self._h, pre_nms_topk_train, post_nms_topk_train), "rs_trainer_set_rpn_topk")

    def write_tensor(self, name: str, data: np.ndarray) -> None:
        """Overwrite a whole trainer tensor (no halo handling)."""
        ptr, dt, shape, _ = self._tensor_ptr(name)
        a = np.ascontiguousarray(data.astype(dt))
        assert a.shape == shape, (a.shape, shape)
        _check(self.lib, self.lib.rs_memcpy_h2d(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes), "rs_memcpy_h2d")

    def backward_trunk(self, n: int) -> None:
        _check(self.lib, self.lib.rs_trainer_backward_trunk(self._h, n), "rs_trainer_backward_trunk")

    def apply_sgd(self, lr: float, momentum: float = 0.9, weight_decay: float = 1e-4) -> None:
        _check(self.lib, self.lib.rs_trainer_apply_sgd(self._h, lr, momentum, weight_decay), "rs_trainer_apply_sgd")

    def overflowed(self) -> bool:
        """True if the last ``apply_sgd`` found inf / nan in the gradient and therefore skipped the step (fp16 loss scale too
        large for that batch).  Synchronises the trainer's stream."""
        return bool(int(self.tensor("grad_overflow")[0]))

    def set_loss_scale(self, loss_scale: float) -> None:
        """fp16 loss scale of the following steps; call it after ``apply_sgd`` (the gradient buffer carries the scale it was
        computed with)."""
        _check(self.lib, self.lib.rs_trainer_set_loss_scale(self._h, float(loss_scale)), "rs_trainer_set_loss_scale")
        self.loss_scale = float(loss_scale)

    def sync(self) -> None:
        _check(self.lib, self.lib.rs_trainer_sync(self._h), "rs_trainer_sync")

    @property
    def param_count(self) -> int:
        return int(self.lib.rs_trainer_param_count(self._h))

    def close(self) -> None:
        if getattr(self, "_infer", None) is not None:
            self._infer.close()
            self._infer = None
        if getattr(self, "_h", None):
            self.lib.rs_trainer_destroy(self._h)
            self._h = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


class MultiScaleTrainer:
    """``INPUT.MIN_SIZE_TRAIN`` with ``MIN_SIZE_TRAIN_SAMPLING: choice`` (R:31-38): one ``Trainer`` per shortest-edge size,
    built lazily.  detectron2 draws the size per image and pads the batch to its largest image: ``select_batch(sizes)`` picks
    the trainer of the largest drawn size (the canvas) and hands it the per-image sizes (``Trainer.set_image_sizes``); with one
    image per GPU that is one size per batch.  The optimiser state follows the batch from trainer to trainer
    (``rs_trainer_copy_state``)."""

    def __init__(self, spec: EngineSpec, weights: Dict[str, np.ndarray], tile_shape: Tuple[int, int, int], sizes: Sequence[int], batch: int = 1,
                 device: int = 0, loss_scale: float = 1024.0, mask_targets: str = "host", wgrad: str = "f32", dgrad: str = "f32",
                 fwd: str = "f32", train_stats: bool = False, freeze_at: int = 2, solver: Optional[SolverOptions] = None):
        if mask_targets not in MASK_TARGET_MODES:
            raise ValueError(f"mask_targets must be one of {MASK_TARGET_MODES}, got {mask_targets!r}")
        _check_wgrad(wgrad, spec)
        _check_dgrad(dgrad, spec)
        _check_fwd(fwd, spec)
        if solver is not None and not isinstance(solver, SolverOptions):
            raise TypeError(f"solver must be a SolverOptions, got {type(solver).__name__}")
        self.solver = solver
        self.freeze_at = _check_freeze_at(freeze_at)
        self.mask_targets = mask_targets
        self.train_stats_on = bool(train_stats)
        self.wgrad = wgrad
        self.dgrad = dgrad
        self.fwd = fwd
        self.spec, self.weights, self.tile_shape, self.batch, self.device, self.loss_scale = spec, weights, tile_shape, batch, device, loss_scale
        self.sizes = [int(s) for s in sizes]
        self._t: Dict[int, Trainer] = {}
        self.current: Optional[Trainer] = None
        self._sampling: Optional[Tuple[int, float, int, float]] = None

    def set_sampling(self, *a) -> None:
        self._sampling = tuple(a)
        for t in self._t.values():
            t.set_sampling(*a)

    def set_wgrad_mode(self, mode: str) -> None:
        _check_wgrad(mode, self.spec)
        self.wgrad = mode
        for t in self._t.values():
            t.set_wgrad_mode(mode)

    def set_dgrad_mode(self, mode: str) -> None:
        _check_dgrad(mode, self.spec)
        self.dgrad = mode
        for t in self._t.values():
            t.set_dgrad_mode(mode)

    def set_fwd_mode(self, mode: str) -> None:
        _check_fwd(mode, self.spec)
        self.fwd = mode
        for t in self._t.values():
            t.set_fwd_mode(mode)

    def set_train_stats(self, on: bool) -> None:
        self.train_stats_on = bool(on)
        for t in self._t.values():
            t.set_train_stats(on)

    def set_solver(self, solver: SolverOptions) -> None:
        """``Trainer.set_solver`` on every trainer, those built later included."""
        if not isinstance(solver, SolverOptions):
            raise TypeError(f"solver must be a SolverOptions, got {type(solver).__name__}")
        self.solver = solver
        for t in self._t.values():
            t.set_solver(solver)

    def grad_norms(self) -> Dict[str, float]:
        """``Trainer.grad_norms`` of the trainer that ran the last step."""
        if self.current is None:
            raise RsError("no trainer has run a step yet")
        return self.current.grad_norms()

    def train_stats(self) -> Dict[str, float]:
        """``Trainer.train_stats`` of the trainer that ran the last step."""
        if self.current is None:
            raise RsError("no trainer has run a step yet")
        return self.current.train_stats()

    def set_loss_scale(self, loss_scale: float) -> None:
        self.loss_scale = float(loss_scale)
        for t in self._t.values():
            t.set_loss_scale(loss_scale)

    def set_rpn_topk(self, pre: int, post: int) -> None:
        """RPN.PRE_NMS_TOPK_TRAIN / POST_NMS_TOPK_TRAIN (R:config/detectron2_config_3bands.yaml:248-250) of every trainer."""
        self._rpn_topk = (int(pre), int(post))
        for t in self._t.values():
            t.set_rpn_topk(*self._rpn_topk)

    def select(self, size: int) -> Trainer:
        """The trainer for shortest-edge ``size``, holding the up-to-date optimiser state."""
        if size not in self._t:
            t = Trainer(self.spec.replace(min_size_test=int(size)), self.weights, self.tile_shape, self.batch, self.device, self.loss_scale,
                        mask_targets=self.mask_targets, wgrad=self.wgrad, dgrad=self.dgrad, fwd=self.fwd, train_stats=self.train_stats_on,
                        freeze_at=self.freeze_at, solver=self.solver)
            if self._sampling:
                t.set_sampling(*self._sampling)
            if getattr(self, "_rpn_topk", None):
                t.set_rpn_topk(*self._rpn_topk)
            self._t[size] = t
        t = self._t[size]
        if self.current is not None and self.current is not t:
            t.copy_state_from(self.current)
        if getattr(t, "_image_sizes", None):
            t.set_image_sizes(None)              # one size for the whole batch unless select_batch says otherwise
        self.current = t
        return t

    def select_batch(self, sizes: Sequence[int]) -> Trainer:
        """The trainer for a batch whose image i was drawn at shortest edge ``sizes[i]``."""
        t = self.select(max(int(s) for s in sizes))
        t.set_image_sizes(list(sizes) if len(set(int(s) for s in sizes)) > 1 else None)
        return t

    @property
    def mask_target_fallbacks(self) -> int:
        """Steps of all the trainers that took the host path because their polygons did not fit the device pool."""
        return sum(t.mask_target_fallbacks for t in self._t.values())

    def net_shape(self, size: int) -> Tuple[int, int]:
        from .spec import resize_shortest_edge_shape
        return resize_shortest_edge_shape(self.tile_shape[0], self.tile_shape[1], int(size), self.spec.max_size_test)

    def close(self) -> None:
        for t in self._t.values():
            t.close()
        self._t.clear()
