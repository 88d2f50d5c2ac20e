/* rs_engine.h -- C ABI of librs_engine.so, the MI355X (gfx950) Mask R-CNN R50-FPN inference engine.
 *
 * Drop-in boundary.  The reference has no FFI for this path: proj-roadsurf calls
 * the STDL object-detector CLI (R:README.md:77-78), whose make_detections.py does, per tile,
 *     outputs = DefaultPredictor(cfg)(cv2.imread(file))        [EXT d2: engine/defaults.py]
 * configured by R:config/config_obj_detec.yaml:74-90 and R:config/detectron2_config_3bands.yaml.
 * rs_engine_infer() replaces exactly that call (batched): HWC uint8 BGR tiles in, per-tile
 * `Instances` fields out (pred_boxes XYXY in tile pixels, scores, pred_classes, pred_masks).
 * Everything behind it -- resize, normalisation, ResNet-50/FPN, RPN, RoIAlign, box head, NMS, mask
 * head, mask paste -- runs as hand-written HIP kernels; there is no CPU fallback.
 *
 * Conventions: plain pointers and sizes, no C++/torch types; every function returns 0 (RS_OK) or
 * a negative error code and sets a message readable through rs_last_error().  An engine belongs
 * to one process and one GPU and is NOT thread-safe.  The caller owns all host buffers; the
 * engine owns its device memory; the weight blob may be freed after rs_engine_create().
 */
#ifndef RS_ENGINE_H
#define RS_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 1
#define RS_SPEC_MAX_LEVELS 5
#define RS_SPEC_MAX_ANCHORS 8
#define RS_NUM_PHASES 3 /* rs_engine_infer_phase: 0 preprocess..RPN proposals, 1 box head..detections, 2 mask head + paste */
#define RS_MASK_SIDE 28 /* 2 * ROI_MASK_HEAD.POOLER_RESOLUTION (R:219) */
#define RS_MAX_CLASSES 80 /* rs_spec.num_classes an inference engine accepts (the COCO model zoo's heads) */
#define RS_TRAIN_MAX_CLASSES 8 /* rs_spec.num_classes rs_trainer_create accepts (RS_ERR_UNSUPPORTED above) */

/* POD mirror of the detectron2 YAML fields the inference path reads
 * (R:config/detectron2_config_3bands.yaml; line numbers per field). */
typedef struct rs_spec {
  int32_t struct_size;            /* sizeof(rs_spec), ABI check */
  int32_t in_channels;            /* len(MODEL.PIXEL_MEAN) :81-84 (3; 4 = RGB+NIR tiles) */
  int32_t flip_channels;          /* INPUT.FORMAT == "RGB" :26 -> reverse the channel axis of the BGR input */
  float pixel_mean[4];            /* :81-84, applied in model-channel order (the BGR-listed quirk is preserved) */
  float pixel_std[4];             /* :85-88 */
  int32_t min_size_test;          /* :30 */
  int32_t max_size_test;          /* :28 */
  int32_t size_divisibility;      /* 32 (FPN) */
  int32_t res_blocks[4];          /* RESNETS.DEPTH 50 -> 3,4,6,3 :100 */
  int32_t stem_out_channels;      /* :110 */
  int32_t res2_out_channels;      /* :108 */
  int32_t stride_in_1x1;          /* :111 */
  int32_t fpn_out_channels;       /* :69 */
  int32_t num_levels;             /* len(RPN.IN_FEATURES) :231-236 */
  int32_t num_anchors;            /* len(ASPECT_RATIOS) x len(SIZES[l]) :45-56 */
  float cell_anchors[RS_SPEC_MAX_LEVELS][RS_SPEC_MAX_ANCHORS][4]; /* generate_cell_anchors, fp32 */
  float anchor_offset;            /* :50 */
  float rpn_bbox_reg_weights[4];  /* :224-228 */
  int32_t rpn_pre_nms_topk;       /* :249 */
  int32_t rpn_post_nms_topk;      /* :247 */
  float rpn_nms_thresh;           /* :245 */
  float rpn_min_size;             /* :90 */
  int32_t num_classes;            /* :191 (CLI overrides from the COCO categories) */
  float box_reg_weights[4];       /* :160-164 */
  float score_thresh_test;        /* :194 / R:config/config_obj_detec.yaml:90 */
  float nms_thresh_test;          /* :190 */
  int32_t detections_per_image;   /* :321 */
  int32_t box_fc_dim;             /* :167 */
  int32_t box_pooler_resolution;  /* :172 */
  int32_t mask_on;                /* :72 */
  int32_t mask_pooler_resolution; /* :219 */
  int32_t mask_num_conv;          /* :218 */
  int32_t mask_conv_dim;          /* :215 */
  float mask_threshold;           /* detector_postprocess default 0.5 */
  float scale_clamp;              /* Box2BoxTransform: log(1000/16) */
  int32_t precision;              /* 0 = production (fp16 operands, fp32 accumulate on MFMA); 1 = fp32 validation mode:
                                     every conv/linear layer in fp32 on the fp32 matrix cores, needs "<layer>.w32" blob entries;
                                     2 = SPLIT OPERANDS (inference engines): reference-equivalent arithmetic on the fp16 matrix
                                     cores -- every GEMM operand as hi + lo fp16 planes (22 significand bits), three products
                                     (hi.hi, hi.lo, lo.hi) into one fp32 accumulator, activations stored as two planes; needs
                                     "<layer>.ws" (fp16 [2][rows][Kpad]: hi rows then lo rows of the weight scaled by a power
                                     of two per row) and "<layer>.wsi" (fp32 [rows]: the inverse scales) blob entries.  The
                                     reference computes in fp32 (no SOLVER.AMP key, R:config/detectron2_config_3bands.yaml:268-305) */
  int32_t batched_nms;            /* appended (RS_SPEC_SIZE_V1 = the struct without it, still accepted and read as 0).
                                     0 = one NMS per category on the boxes as they are (RPN: per level; box head: per class);
                                     1 = torchvision 0.11's batched_nms size rule, per image and NMS stage: when at most 1000 boxes enter the call
                                     (boxes.numel() <= 4000) every box is shifted by category * (largest coordinate + 1) in fp32 before the IoUs
                                     are computed, as `_batched_nms_coordinate_trick` does ([EXT tv: ops/boxes.py]); above 1000 as mode 0 */
} rs_spec;
#define RS_SPEC_SIZE_V1 ((int32_t)offsetof(rs_spec, batched_nms))
/* The batched_nms mode a spec block selects: 0 for a caller compiled against the struct without the field (struct_size ==
 * RS_SPEC_SIZE_V1), the field's value for the current struct; RS_ERR_ARG (negative) for any other struct_size or value.  Host only. */
int rs_spec_batched_nms(const rs_spec* spec);

/* Caller-allocated result block for n tiles, D = detections_per_image slots per tile.
 * Entries [0, count[i]) of tile i are valid and sorted by score (descending). Any pointer except
 * `count` may be NULL to skip that field. */
typedef struct rs_dets {
  int32_t* count;     /* [n] */
  float* boxes;       /* [n][D][4]  x1,y1,x2,y2 in tile pixels   (Instances.pred_boxes) */
  float* scores;      /* [n][D]                                  (Instances.scores) */
  int32_t* classes;   /* [n][D]     0-based contiguous class id  (Instances.pred_classes) */
  uint8_t* masks;     /* [n][D][h][ceil(w/8)] bit-packed rows, bit b of a byte = pixel 8*byte+b
                         (Instances.pred_masks, >= mask_threshold) */
  float* mask_probs;  /* [n][D][28][28] sigmoid probabilities before pasting; rows at or past count[i] are unspecified (zero or an earlier batch's values) */
} rs_dets;

/* Detection masks cropped to their boxes (a pasted mask is zero outside its box): what the streaming host interface copies
 * instead of the full canvases -- 100 x h x ceil(w/8) bytes per tile (3.3 MB at 512x512, 13 MB at 1024x1024) shrink to the
 * boxes' area.  Crop (i, d) covers byte columns [rects[0], rects[0] + rects[2]) and rows [rects[1], rects[1] + rects[3]) of
 * the bit-packed canvas rs_dets.masks describes, rows stored back to back at data + offsets[i][d]; crops follow each other
 * in (tile, slot) order.  Caller-allocated (pinned memory recommended); capacity n*D*h*ceil(w/8) always suffices. */
typedef struct rs_mask_crops {
  int32_t* rects;      /* [n][D][4]: first byte column, first row, bytes per row, rows; zeros for empty slots */
  uint32_t* offsets;   /* [n][D] */
  uint8_t* data;
  uint64_t capacity;   /* bytes available at data */
  uint64_t used;       /* out (rs_engine_fetch_crops_wait): bytes written */
} rs_mask_crops;

typedef struct rs_engine rs_engine;

/* Build an engine for tiles of one fixed shape (h, w, c) and batches of up to max_batch tiles.
 * `weights` is the blob written by proj_roadsurf_amd.weights.pack_weights() (see "weight blob").
 * `stream` is a hipStream_t to run on, or NULL to let the engine create its own. */
int rs_engine_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal,
                     int max_batch, int tile_h, int tile_w, int tile_c, void* stream, rs_engine** out);
void rs_engine_destroy(rs_engine* e);

/* DefaultPredictor.__call__ for n tiles: tiles = [n][h][w][c] uint8, channel order as cv2.imread
 * returns it (BGR).  Host buffers; does H2D, the forward, D2H, and waits. */
int rs_engine_infer(rs_engine* e, const uint8_t* tiles_host, int n, rs_dets* out_host);

/* Same forward with tiles already resident in device memory; enqueues on the engine's stream and
 * returns without waiting.  Results stay on the device until rs_engine_fetch(). */
int rs_engine_infer_device(rs_engine* e, const uint8_t* tiles_dev, int n);
int rs_engine_sync(rs_engine* e);
int rs_engine_fetch(rs_engine* e, int n, rs_dets* out_host);

/* The same forward, enqueued one phase at a time (phase 0, 1, 2 in order, same tiles/n for all three) so that a
 * caller driving TWO engines created on one shared `stream` can interleave them: the latency-bound detection glue
 * at the end of phases 0 and 1 runs on an engine-private side stream and is hidden behind the other engine's
 * convolutions, which stay serialised on the shared stream.  Enqueue order per batch k (engine k mod 2):
 *   phase0(k), phase2(k-1), phase1(k)          -- see proj_roadsurf_amd/engine.py:LanePipeline
 * rs_engine_infer_device(e, t, n) == phases 0, 1, 2 back to back.  There is no reference counterpart
 * (DefaultPredictor is synchronous, one image per call: [EXT d2: engine/defaults.py]). */
int rs_engine_infer_phase(rs_engine* e, const uint8_t* tiles_dev, int n, int phase);
int rs_engine_phase_count(void);
/* Diagnostic (tools/parity/lanes_stress3.py): enqueue only the stages whose name contains `substr`, on the engine's stream, on the data of the last forward. */
int rs_debug_run_stages_matching(rs_engine* e, const char* substr, int n);

/* Asynchronous host interface (what a streaming caller -- make_detections.py over a tile list -- uses instead of rs_engine_infer):
 * pinned host memory, the upload enqueued on the engine's stream in front of the forward, and the results copied back on a
 * separate copy stream behind an event, so batch k's device-to-host copy (3.3 MB of packed masks per 512x512 tile) overlaps batch
 * k+1's forward.  With two engines on one shared stream (rs_engine_infer_phase) call rs_engine_fetch_async right after the
 * engine's phase 2 has been enqueued.  Buffers given to upload/fetch_async must come from rs_host_alloc and stay untouched until
 * rs_engine_fetch_wait returns. */
void* rs_host_alloc(size_t nbytes);
void rs_host_free(void* p);
/* Pin / unpin an existing host allocation (e.g. a shared-memory slab that decoder processes fill) so that rs_engine_upload_async
 * copies straight out of it; the caller keeps the bytes unchanged until the forward that consumes them has delivered its results. */
int rs_host_register(void* p, size_t bytes);
int rs_host_unregister(void* p);
int rs_engine_upload_async(rs_engine* e, const uint8_t* tiles_host, int n);
int rs_engine_fetch_async(rs_engine* e, int n, rs_dets* out_host);
int rs_engine_fetch_wait(rs_engine* e);
/* The same two calls with the masks as crops: rs_engine_fetch_crops_async enqueues, on the copy stream behind the forward, the
 * crop planning + compaction kernels and the copies of count / boxes / scores / classes (dets->masks and ->mask_probs are
 * ignored) and of the crop table; rs_engine_fetch_crops_wait waits for them, then copies exactly `used` bytes of crop data
 * and waits for that copy.  The engine's result buffers are free for the next forward after the first step. */
int rs_engine_fetch_crops_async(rs_engine* e, int n, rs_dets* dets_host, rs_mask_crops* crops_host);
int rs_engine_fetch_crops_wait(rs_engine* e, rs_mask_crops* crops_host);

/* Stream the engine launches on (hipStream_t), for event timing by the caller. */
void* rs_engine_stream(rs_engine* e);

/* Per-stage timing with HIP events on the engine's stream.  mode 0 = off; 1 = record + wait per
 * stage (serialises the host, debugging); 2 = record only, events are read back when
 * rs_engine_stage_info() is next called (up to 32 forwards' worth; extra forwards are not timed);
 * 3 = like 2 but only every 4th forward is bracketed (the others replay the captured hipGraph). */
int rs_engine_set_profiling(rs_engine* e, int mode);
int rs_engine_stage_count(rs_engine* e);
/* name_out: >= 96 bytes.  ms_total / calls accumulate since the last rs_engine_set_profiling().
 * flops = algorithmic FLOPs of one call at the last batch size (0 for non-GEMM stages),
 * bytes = algorithmic HBM bytes of one call (inputs read once + outputs written once). */
int rs_engine_stage_info(rs_engine* e, int i, char* name_out, double* ms_total, int* calls, double* flops, double* bytes);
/* Saturation counts: elements that a stage clamped to the fp16 range (NaN or |value| > 65504 where it rounds an fp32 value to fp16;
 * DESIGN.md 3.6) in the most recent forward whose results have been fetched (rs_engine_infer, rs_engine_fetch, or rs_engine_fetch_wait /
 * rs_engine_fetch_crops_wait after the matching *_async).  counts[i] for stage i (names: rs_engine_stage_info), i < min(cap, stage count);
 * returns the stage count (< 0 on error).  Stages that store fp32 (every stage of precision 1) always report 0. */
int rs_engine_saturation(rs_engine* e, int64_t* counts, int cap);
/* Kernel symbol (tile variant) the stage's last call launched, "" for non-GEMM stages. name_out: >= 96 bytes. */
int rs_engine_stage_kernel(rs_engine* e, int i, char* name_out);
/* Tile-variant number of the stage's last call (-2 = not a GEMM stage, -1 = fp32 kernel; numbering: rs_op_conv_variant). */
int rs_engine_stage_variant(rs_engine* e, int i);

/* Intermediate tensors by name (parity tests): device pointer, dtype (1 f16, 2 f32, 3 i32, 4 u8, 5 = two fp16 planes of the
 * given shape back to back, value = plane 0 + plane 1: activations of precision 2),
 * up to 5 dims (dims[ndim..] = 1) and the spatial halo of NHWC activations. */
int rs_engine_tensor(rs_engine* e, const char* name, void** dev_ptr, int* dtype, int* ndim, int64_t dims[5], int* halo);
int rs_engine_tensor_count(rs_engine* e);
int rs_engine_tensor_name(rs_engine* e, int i, char* name_out /* >= 96 bytes */);

/* Network input geometry chosen by ResizeShortestEdge for this tile shape. */
int rs_engine_net_shape(rs_engine* e, int* resized_h, int* resized_w, int* padded_h, int* padded_w);

/* -------- stand-alone operators on caller-owned device memory (unit parity tests) -------- */

/* NHWC fp16 convolution / GEMM with fused epilogue.  in: [n][hi+2*in_halo][wi+2*in_halo][cin],
 * w: [cout_rows][kpad] fp16 (k = (kh,kw,cin), cin fastest, kpad multiple of 64), bias fp32,
 * out: [n][ho+2*out_halo][wo+2*out_halo][cout] fp16, or fp32 when out_f32.
 * residual (optional) has the geometry of out; upsample_add (optional) is
 * [n][ho/2+2*out_halo][wo/2+2*out_halo][cout] and is added at (y/2, x/2).
 * variant: -1 auto, 0 = 128x128 tile, 1 = 256x64, 2 = 256x16 (fp32 out), 3 = 256x128, 4 = 256x256, 7 = 64x128,
 * 8 = 128x64, 9 = 32x128, 10 = 64x256, 12 = conv_deep 256x256 (pixels x channels).  use_glds: 1 = direct
 * global->LDS staging (production), 0 = register staging (cross-check). */
int rs_op_conv2d(const void* in, const void* w, const float* bias, void* out, const void* residual,
                 const void* upsample_add, int n, int hi, int wi, int cin, int in_halo, int kh, int kw,
                 int stride, int pad, int cout, int kpad, int out_halo, int relu, int out_f32, int deconv2x,
                 int variant, int use_glds, void* stream);

/* Fused tail of an identity-shortcut bottleneck block of the 64-wide stage (csrc/bneck_fused.hip): t2 = relu(conv3x3(t1, w2) + b2),
 * out = relu(w3 . t2 + b3 + x), and -- when w1p is given -- t1n = relu(w1 . out + b1), the next block's conv1, in one launch
 * ([EXT d2: modeling/backbone/resnet.py BottleneckBlock.forward]).  All maps NHWC fp16 with a zero halo of 1: t1 / t1n
 * [n][h+2][w+2][64], x / out [n][h+2][w+2][256].  w2 [64][576] (kh, kw, cin); w3p [256][64] and w1p [64][256] with their K columns
 * in the register-chaining order (weights.py _perm_k64); biases fp32.  Projection-shortcut form (first block of the stage): x =
 * NULL and instead x0 [n][h+2][w+2][64], the shortcut's input, with wsc [256][64] (natural K order); b3 then is conv3's plus the
 * shortcut's bias: out = relu(w3 . t2 + wsc . x0 + b3). */
int rs_op_bneck_tail(const void* t1, const void* w2, const float* b2, const void* w3p, const float* b3, const void* x, void* out,
                     const void* w1p, const float* b1, void* t1n, const void* x0, const void* wsc, int n, int h, int w, int width,
                     void* stream);     /* width: 64 (as written above) or 128 (every 64 / 256 / 576 above doubled; no projection form) */

/* The identity-shortcut form of rs_op_bneck_tail in the split-operand precision mode (csrc/bneck_split.hip; rs_spec.precision == 2): every map is
 * a hi plane with its lo plane `*_lo` ELEMENTS behind it (value = hi + lo); every weight is [2 * rows][K] fp16 -- hi rows, then lo rows, of the
 * fp32 weight with each row scaled by a power of two (weights.py split_planes) -- and s2 / s3 / s1 hold the inverse scales per row.  Same shapes,
 * K orders and halo as rs_op_bneck_tail; w1p (with s1, b1, t1n) may be NULL.  Projection-shortcut form (width 64 only): x = NULL and x0
 * [n][h+2][w+2][64] (+ x0_lo) is the shortcut's input; w3p then is [2 * 256][128] -- the K columns of conv3 in the chained order followed by
 * the shortcut's 64 in natural order, ONE scale per row over both (s3) -- and b3 the sum of the two biases:
 * out = relu((w3 . t2 + wsc . x0) * s3 + b3). */
int rs_op_bneck_tail_split(const void* t1, int64_t t1_lo, const void* w2, const float* s2, const float* b2, const void* w3p, const float* s3,
                           const float* b3, const void* x, int64_t x_lo, void* out, int64_t out_lo, const void* w1p, const float* s1,
                           const float* b1, void* t1n, int64_t t1n_lo, const void* x0, int64_t x0_lo, int n, int h, int w, int width,
                           void* stream);

/* Raster voting: the overlay of R:scripts/road_segmentation/determine_class.py:97-120 on the tile grid.
 * det_masks [n_det][h][ceil(w/8)] and label_masks [n_labels][same] are bit-packed device buffers (rs_dets.masks layout; h*ceil(w/8)
 * must be a multiple of 4); inter [n_labels][n_det] receives the pixel count of every (label, detection) intersection, label_area
 * [n_labels] every label's own pixel count (device buffers).  rs_engine_label_overlap runs it on the masks of tile `tile` of the
 * engine's last forward (n_det = D slots; only the first count[tile] columns are meaningful) on the engine's stream. */
int rs_op_mask_overlap(const uint8_t* det_masks, int n_det, const uint8_t* label_masks, int n_labels, int h, int w, int32_t* inter,
                       int32_t* label_area, void* stream);
int rs_engine_label_overlap(rs_engine* e, int tile, const uint8_t* label_masks_dev, int n_labels, int32_t* inter_dev, int32_t* label_area_dev);

/* The tile variant launch_conv would pick for a conv / linear layer of this shape (no launch, no GPU needed): m = batch *
 * Ho * Wo output pixels, k x k taps over cin channels (+ cin2 channels of a second 1x1 K source, 0 = none), cout channels,
 * deconv2x as in rs_op_conv2d.  The choice depends on m, i.e. on the batch size: tests enumerate it per layer and batch
 * (tests/test_host_cpu.py::test_conv_variant_table).  Also returns the number of LDS K-step buffers in *stages_out. */
int rs_op_conv_variant(int m, int cin, int k, int cout, int cin2, int deconv2x, int out_f32, int* stages_out);

/* The same rule in the split-operand precision mode, which also depends on the stride; deconv_predict = 1: the mask head's fused deconv 2x2 s2 +
 * predictor over m input pixels (4 * cout rows), as the engine launches it. */
int rs_op_conv_variant_split(int m, int cin, int k, int stride, int cout, int cin2, int deconv_predict, int* stages_out);

/* Diagnostic builds only (csrc compiled with -DRS_CLOCK_PROBE, tools/ubench/clock_probe.py): device buffer of 2 int64 per
 * workgroup that rs_op_conv2d's 256x256 deep-prefetch kernel fills with {shader clocks, 100 MHz ticks} spent in its K loop.
 * No effect in the production build. */
int rs_debug_set_conv_probe(void* buffer);

/* Saturation counter of the calling thread's stand-alone operators (rs_op_conv2d, rs_op_conv2d_split, rs_op_conv2d_dual, rs_op_bneck_tail,
 * rs_op_bneck_tail_split): while non-null, each such call adds the number of elements it clamped to the fp16 range into *(uint64_t*)dev_u64 (device
 * memory).  Null (the default) = not counted. */
int rs_op_set_saturation_counter(void* dev_u64);

/* rs_op_conv2d in the split-operand precision mode (rs_spec.precision == 2): `in`, `w`, `out`, `residual`, `upsample_add` point to
 * the hi plane of an fp16 tensor whose lo plane lies `*_lo` ELEMENTS behind it (value = hi + lo); w holds the weight rows scaled
 * by a power of two per row, wscale[rows] the inverse scales.  out_f32 = 1: one fp32 output as in rs_op_conv2d. */
int rs_op_conv2d_split(const void* in, int64_t in_lo, const void* w, int64_t w_lo, const float* wscale, const float* bias, void* out, int64_t out_lo,
                       const void* residual, int64_t res_lo, const void* upsample_add, int64_t up_lo,
                       int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad,
                       int out_halo, int relu, int out_f32, int deconv2x, int variant, void* stream);

/* The mask head's fused deconv 2x2 s2 + ReLU + predictor in the split-operand mode on caller tensors: in [entries][side + 2][side + 2][256] (halo 1), w [1024][256]
 * (rows (dy, dx, cout), scaled; wscale / bias [1024]), dot_w [classes][256] fp32, slot[entry] the row of logits [slots][2 side][2 side] an entry writes, cls[slot] its
 * class; only min(entries, *count_dev) entries run.  variant 14 / 10 / 0 ADD into logits (zero them first); 28 (29 / 30 / 31: 64 / 128 / 256-pixel tiles) store them. */
int rs_op_deconv_predict_split(const void* in, int64_t in_lo, const void* w, int64_t w_lo, const float* wscale, const float* bias, const float* dot_w, int classes,
                               const int32_t* cls, const int32_t* slot, const int32_t* count_dev, float* logits, int entries, int side, int variant, void* stream);

/* Bottleneck output with a projection shortcut as ONE GEMM over two activation sources:
 *   out = act( conv_khxkw(in; W[:, :kh*kw*cin]) + conv_1x1_stride2(in2; W[:, kh*kw*cin:]) + bias )
 * i.e. BottleneckBlock.forward's `out = conv3(out); shortcut = self.shortcut(x); out += shortcut; relu`
 * ([EXT d2: modeling/backbone/resnet.py BottleneckBlock.forward]) with both FrozenBN-folded convolutions'
 * weights concatenated along K and their biases added.  in2: [n][h2+2*in2_halo][w2+2*in2_halo][cin2] fp16;
 * output pixel (y, x) reads in2 pixel (y*stride2, x*stride2). */
int rs_op_conv2d_dual(const void* in, const void* in2, const void* w, const float* bias, void* out,
                      int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad,
                      int h2, int w2, int cin2, int in2_halo, int stride2,
                      int cout, int kpad, int out_halo, int relu, int variant, void* stream);

/* Training path: input gradient of rs_op_conv2d's convolution, with the backward epilogue fused:
 *   dx = relu'(mask) * ( conv_transpose(dy, W) + res + res32 + sum2x2(down) )
 * dy: [n][ho+2h][wo+2h][cout] fp16; w_t: the transposed, tap-flipped weight [cin][(kh-1-i, kw-1-j, co)] fp16 (kpad columns);
 * dx/res/mask: [n][hi+2h][wi+2h][cin] fp16, res32 the same geometry in fp32, down: [n][2hi+2h][2wi+2h][cin] fp16 (all
 * optional except dx).  stride 1, or stride s with a 1x1 kernel (STRIDE_IN_1X1, R:config/detectron2_config_3bands.yaml:111):
 * then dx is only written at every s-th pixel and the caller provides zeros elsewhere.  What autograd reaches through
 * cuDNN backward-data + the ReLU / add / nearest-upsample backward nodes ([EXT d2: modeling/backbone/{resnet,fpn}.py]). */
int rs_op_conv2d_dgrad(const void* dy, const void* w_t, void* dx, const void* res, const float* res32, const void* mask,
                       const void* down, int n, int hi, int wi, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                       int pad, int kpad, int halo, int variant, void* stream);
/* The same input gradient for the reference-precision trainer with the product on the fp16 matrix cores ("input gradients on
 * split operands").  Every tensor is fp32: dy, w_t [cin][kpad], dx, res, res32, mask (the saved activation, > 0 passes), down.  For the
 * life of the call it allocates scratch, takes the abs-max of dy on the device (integer maximum, no read-back), writes
 * hi = fp16(dy 2^e), lo = fp16(dy 2^e - hi) with e = 14 - floor(log2 amax) (0 for a zero or non-finite dy), splits w_t by rows
 * (rs_op_split_rows) and runs three v_mfma_f32_16x16x32_f16 products (hi.lo, hi.hi, lo.hi) into one fp32 accumulator:
 *   dx = mask( acc * inv_scale[row] * 2^-e + res + sum2x2(down) + res32 ),  stored fp32; two calls give the same bits.  Per element
 *   |gemm - exact| <= 2^-20 sum|dy||w| + 2^-36 T max|dy| rowmax|w| + (the accumulation-order error of the fp32 kernel), T = kh kw cout.
 * variant: -1 = the library's rule, or a tile by number: 7 (64 x 128), 14 (128 x 256), 4 (256 x 256; cin a multiple of 128 resp. 256) or
 * 2 (256 x 16).  count_dev: optional device int, images computed = min(n, *count_dev), the others are not written.
 * Refused before a device is touched, with the entry's name in rs_last_error: null dy / w_t / dx (RS_ERR_ARG), n < 1, cout (the K side) no
 * multiple of 64, a halo below k - 1 - pad (RS_ERR_ARG), stride > 1 with a kernel that is not 1x1 (RS_ERR_UNSUPPORTED).
 * rs_op_conv2d_dgrad_split_serves: 1 when a layer of this shape runs split (in the operator and in the trainer's mode), else 0: cin a
 * multiple of 16, cout of 64, stride 1 or a 1x1 kernel.  Host only. */
int rs_op_conv2d_dgrad_split(const void* dy, const void* w_t, void* dx, const void* res, const float* res32, const void* mask,
                       const void* down, int n, int hi, int wi, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                       int pad, int kpad, int halo, int variant, const int32_t* count_dev, void* stream);
int rs_op_conv2d_dgrad_split_serves(int cin, int cout, int kh, int stride);
/* The forward convolution / linear layer of the reference-precision trainer with the product on the fp16 matrix cores (DESIGN.md 8,
 * "forward on split operands").  Every tensor is fp32: x [n][hi+2*in_halo][wi+2*in_halo][cin], w [cout][kpad] in the engine's layout
 * (k = (kh, kw, cin), cin fastest; the FrozenBN scale already folded), bias [cout], y [n][ho+2*out_halo][wo+2*out_halo][cout] with
 * ho = (hi + 2 pad - kh) / stride + 1, res (optional) in y's geometry, up (optional) [n][(ho+1)/2+2*out_halo][(wo+1)/2+2*out_halo][cout],
 * added at (y >> 1, x >> 1).  For the life of the call it allocates scratch, takes the abs-max of x on the device (integer maximum, no
 * read-back), writes hi = fp16(x 2^e), lo = fp16(x 2^e - hi) with e = 14 - floor(log2 amax) (0 for a zero or non-finite x), splits w
 * by rows (rs_op_split_rows) and runs three v_mfma_f32_16x16x32_f16 products (hi.lo, hi.hi, lo.hi) into one fp32 accumulator:
 *   y = relu?( acc * inv_scale[row] * 2^-e + bias + res + up ),  stored fp32; two calls give the same bits.  Per element
 *   |gemm - exact| <= 2^-20 sum|x||w| + 2^-36 T max|x| rowmax|w| + (the accumulation-order error of the fp32 kernel), T = kh kw cin.
 * stride is the input stride of the taps, any kernel size (the 1x1 stride-2 layers of res3..res5 are the model's case).
 * variant: -1 = the library's rule, or a tile by number: 7 (64 px x 128 rows), 14 (128 x 256), 4 (256 x 256; cout a multiple of 128
 * resp. 256) or 2 (256 x 16).  count_dev: optional device int, images computed = min(n, *count_dev), the others are not written.
 * Refused before a device is touched, with the entry's name in rs_last_error (RS_ERR_ARG): null x / w / bias / y, n < 1, cin (the K
 * side) no multiple of 64, cout (the rows) no multiple of 16, an input halo below the pad, a kernel that is not square, a kpad below
 * kh kw cin or no multiple of 64.
 * rs_op_conv2d_fwd_split_serves: 1 when a layer of this shape runs split (in the operator and in the trainer's mode), else 0: cout a
 * multiple of 16, cin of 64.  The stem (cin 3 / 4) and the mask deconvolution are not served.  Host only. */
int rs_op_conv2d_fwd_split(const void* x, const void* w, const float* bias, void* y, const void* res, const void* up, int n, int hi,
                           int wi, int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad, int out_halo,
                           int relu, int variant, const int32_t* count_dev, void* stream);
int rs_op_conv2d_fwd_split_serves(int cin, int cout, int k, int stride);
/* Rows of a device fp32 matrix w [rows][k] as fp16 planes [2 * rows][k] (the hi rows, then the lo rows) of w 2^e(row), with
 * inv_scale[row] = 2^-e(row): e = 13 - floor(log2 max|row|) clipped to [-100, 100], so the row maximum lies in [2^13, 2^14) (0 for a
 * zero or non-finite row) -- bit for bit weights.split_planes.  The row maximum is an integer maximum over the bits of |w|. */
int rs_op_split_rows(const float* w, int rows, int k, void* planes, float* inv_scale, void* stream);

/* Training path: weight gradient of rs_op_conv2d's convolution (conv_wgrad.hip),
 *   grad[co][(kh,kw,ci)] = scale[co] * sum_{n,y,x} dy[n][y][x][co] * in[n][y*stride+kh-pad][x*stride+kw-pad][ci]
 * -- what autograd computes for Conv2d.weight / Linear.weight ([EXT d2: layers/wrappers.py Conv2d]; with FrozenBN the
 * trainable tensor is the unfolded weight, hence the optional per-channel `scale`).  dy: [n][ho+2*dy_halo][wo+2*dy_halo][cout]
 * fp16 with a zero halo; grad: fp32 [cout][kpad] in the forward weight layout.  splits <= 0: chosen by the library. */
int rs_op_conv2d_wgrad(const void* dy, const void* in, float* grad, const float* scale, int n, int hi, int wi, int cin,
                       int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits,
                       void* stream);
/* the same from fp32 operands (dy, x point to float): the reference-precision trainer's conv_wgrad_f32_kernel */
int rs_op_conv2d_wgrad_f32(const void* dy, const void* in, float* grad, const float* scale, int n, int hi, int wi, int cin,
                       int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits,
                       void* stream);
/* the same fp32 operands and fp32 result with the product on the fp16 matrix cores ("weight gradients on split operands"):
 * each operand is scaled by one power of two per call (abs-max pass on the device, no read-back) and split into hi + lo fp16 planes,
 * three v_mfma_f32_16x16x32_f16 products (hi.lo, hi.hi, lo.hi) go into one fp32 accumulator, the scale is undone exactly and the fixed-order
 * reduction of the other two operators follows: two calls give the same bits.  Per element
 *   |result - exact| <= 2^-20 sum|dy||in| + 2^-36 M max|dy| max|in| + (the accumulation-order error of rs_op_conv2d_wgrad_f32).
 * Allocates its plane scratch for the call; null operands and bad geometry are refused (RS_ERR_ARG) before a device is touched.
 * rs_op_conv2d_wgrad_split_serves: 1 when a layer of these channel counts runs on the fp16 matrix cores, 0 when the call (and the
 * trainer's split mode) falls through to the fp32 kernel for it -- channel counts that are no multiple of 8.  Host only. */
int rs_op_conv2d_wgrad_split(const void* dy, const void* in, float* grad, const float* scale, int n, int hi, int wi, int cin,
                       int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits,
                       void* stream);
int rs_op_conv2d_wgrad_split_serves(int cin, int cout);

/* Backward of the stem (stem_bwd.hip; a trainer with freeze_at 0 runs both).
 * rs_op_maxpool3x3s2_bwd: gradient of max_pool2d(3, 2, 1) fused with the ReLU mask of the pool's input,
 *   dx[n][iy][ix][c] = (x[n][iy][ix][c] > 0) * sum of dq[n][oy][ox][c] over the windows (oy, ox) whose argmax is (iy, ix).
 * x: [n][hc+2*x_halo][wc+2*x_halo][c] the pool's input (post-ReLU), dq: [n][hq+2*q_halo][wq+2*q_halo][c] with hq = (hc-1)/2+1,
 * wq = (wc-1)/2+1, dx: x's geometry; fp16, or float with f32 != 0; c a multiple of 8 (fp16) or 4 (fp32).  The argmax is ATen's
 * (max_pool2d_with_indices): the window is scanned in (row, column) order, a later element replaces the current one only if it is
 * strictly greater or NaN, padding positions never win.  The at most four windows of a pixel are summed in fp32 in ascending
 * (oy, ox) order, ATen's CPU scatter order, so the result is defined bit for bit (fp16: one final rounding).  No atomics; every
 * interior element of dx is written, the halo of no tensor is read or written. */
int rs_op_maxpool3x3s2_bwd(const void* x, const void* dq, void* dx, int n, int hc, int wc, int c, int x_halo, int q_halo, int f32,
                           void* stream);
/* rs_op_stem_wgrad: weight gradient of the 7x7 stride-2 pad-3 stem convolution,
 *   grad[co][(kh,kw,ci)] = scale[co] * sum_{n,y,x} dy[n][y][x][co] * x0[n][2y+kh-3][2x+kw-3][ci]
 * in the stem's forward GEMM layout: fp32 [64][256], column (kh * 8 + kw) * 4 + ci (taps padded 7 -> 8 per row, channels to 4, K to
 * 256).  The padding columns -- kw = 7, columns >= 224, ci >= cin -- are written as exact zeros.  dy: [n][hc+2*dy_halo][wc+2*dy_halo][64],
 * x0: [n][2*hc+2*x_halo][2*wc+2*x_halo][4] with x_halo >= 3; both fp16 (rs_op_stem_wgrad) or both float (rs_op_stem_wgrad_f32).
 * Exact products, fp32 accumulation, the pixel axis split into `splits` partial sums (<= 0: chosen by the library, at most 512) that
 * are added in a fixed order: two calls give the same bits.  scale: [64] or null. */
int rs_op_stem_wgrad(const void* dy, const void* x0, float* grad, const float* scale, int n, int hc, int wc, int cin, int dy_halo,
                     int x_halo, int splits, void* stream);
int rs_op_stem_wgrad_f32(const void* dy, const void* x0, float* grad, const float* scale, int n, int hc, int wc, int cin, int dy_halo,
                         int x_halo, int splits, void* stream);

/* Greedy NMS over `segments` independent lists of up to `cap` (<= 2048) boxes in priority order
 * (torchvision.ops.nms: suppress when the fp32 IoU > thresh). keep: [segments][cap] 0/1.
 * The kernels compare the fp32 IoU with `thresh` in fp32.  torchvision compares it with a double threshold t; a
 * caller who wants that gets it by passing the largest float <= t (for a float IoU x, x > t exactly when x exceeds
 * that float).  RsSpec.rpn_nms_thresh and nms_thresh_test are read the same way; the Python binding
 * (make_rs_spec) writes them so.
 * Dispatch follows the engine's: the suppression mask lives in global memory at cap > 1024, and at cap <= 1024
 * with <= 32 segments (rows shared by several workgroups, the scan in a second launch); in LDS otherwise. */
int rs_op_nms(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep,
              int segments, int cap, float thresh, void* stream);
/* torchvision.ops.batched_nms over `images` independent calls of `segments_per_image` categories each: boxes / valid / keep
 * [images][segments_per_image][cap]..., counts [images][segments_per_image].  rule = 0: rs_op_nms over all segments.  rule = 1: the
 * size rule of rs_spec.batched_nms = 1, decided per image on the device from the number of valid boxes; launches and dispatch as in
 * the engine's rpn.nms / box.nms stages; cap must exceed 1000 (the engine's are 1024 and 2048).  rs_op_batched_nms_decision is the
 * same call and also hands out what the kernel decided (optional device buffers, rule = 1 only): rule_out [images][2] = {taken, boxes
 * that enter the call}, unit_out [images] = fl(largest coordinate + 1) where taken, else 0 -- the engine's *_nms_rule / *_nms_unit. */
int rs_op_batched_nms(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep, int images,
                      int segments_per_image, int cap, float thresh, int rule, void* stream);
int rs_op_batched_nms_decision(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep, int images,
                               int segments_per_image, int cap, float thresh, int rule, int32_t* rule_out, float* unit_out, void* stream);

/* The engine's box.merge_postprocess stage alone (fast_rcnn_inference's top-k over the NMS survivors of all classes, then
 * detector_postprocess's box part), on device buffers laid out as the engine's: dec_boxes [images][cap][num_classes][4] and dec_scores
 * [images][cap][num_classes] (cap <= 1024 RoI slots per image), seg_roi / keep [images][num_classes][1024] (candidates of a class in
 * NMS order: RoI slot, keep flag), seg_count [images][num_classes].  Per image the kept entries are ordered by score descending, ties by
 * lower roi * num_classes + class first, and the first dets_per_image (<= 1024) are taken; each box is scaled by (scale_x, scale_y),
 * clipped to [0, out_w] x [0, out_h] and dropped when empty.  Outputs per image, packed to the front: det_boxes_net (unscaled boxes),
 * det_boxes, det_scores, det_classes, det_roi (optional), det_count.  1 <= num_classes <= RS_MAX_CLASSES: up to 8 classes one launch,
 * above it the two-launch form of the engine (groups of 8 classes, then their partial winners). */
int rs_op_det_merge(const float* dec_boxes, const float* dec_scores, const int32_t* seg_roi, const int32_t* seg_count, const uint8_t* keep,
                    int images, int num_classes, int cap, int dets_per_image, float scale_x, float scale_y, float out_w, float out_h,
                    float* det_boxes_net, float* det_boxes, float* det_scores, int32_t* det_classes, int32_t* det_roi, int32_t* det_count,
                    void* stream);

/* ROIPooler + ROIAlign(aligned=True, sampling_ratio=0) over up to 4 NHWC fp16 levels (halo 1,
 * 256 channels). rois: [n_rois][4] image coordinates, batch_index = roi / rois_per_image.
 * out: [n_rois][P+2*out_halo][P+2*out_halo][256] fp16; levels_out optional [n_rois]. */
int rs_op_roi_align(const void* const feats[4], const int32_t heights[4], const int32_t widths[4],
                    const float scales[4], int nlevels, const float* rois, int n_rois, int rois_per_image,
                    int P, int out_halo, void* out, int32_t* levels_out, void* stream);

/* Training path: adjoint of rs_op_roi_align.  dout: gradient of the pooled output, same layout as `out` above;
 * dfeats[l]: fp32 gradient maps with the geometry of feats[l] ([N][H_l+2][W_l+2][256]), ACCUMULATED into.  Owner-computes: one workgroup
 * per 8 x 8-cell region adds the RoIs that reach it in entry order (fixed summation order, reproducible bits); RoIs whose window exceeds
 * the weight tables go through float atomics, as every RoI does in torchvision's roi_align_backward_kernel
 * ([EXT tv: csrc/ops/cuda/roi_align_kernel.cu]).  Synchronises `stream` (its table workspace lives for the call). */
int rs_op_roi_align_bwd(float* const dfeats[4], const int32_t heights[4], const int32_t widths[4], const float scales[4],
                        int nlevels, const float* rois, int n_rois, int rois_per_image, int P, int out_halo, const void* dout,
                        void* stream);

/* The two RoIAlign operators with every form the engine and the trainer launch (same launchers, same kernels).
 *  precision     0: fp16 maps and output; 1: fp32 maps and output (per-sample kernel); 2: split operands -- feats[l] / out are the hi
 *                fp16 planes, the lo planes lie feat_lo[l] / out_lo ELEMENTS behind them.
 *  n_entries_cap entries launched (the grid); out / dout: [n_entries_cap][P+2*out_halo]^2[256].  Entry e pools slot slot_list[e] (e itself
 *                when slot_list is null) of rois [n_images * slots_per_image][4]; image = slot / slots_per_image.
 *  n_entries     optional device int: entries past min(*n_entries, n_entries_cap) are neither read nor written.
 *  per_image_count  optional device [n_images]: a slot whose rank in its image is >= the count is empty -- the forward writes zeros
 *                (both planes), the backward nothing.
 *  order         optional device permutation of [0, n_entries_cap): the order the windowed forward visits the entries in; every entry
 *                still lands in its own slot of `out`.
 *  grad_f32      backward: dout is float (1) or fp16 (0).
 * RS_ROI_WINDOW / RS_ROI_BWD_ATOMIC choose between the kernel forms as in the engine. */
int rs_op_roi_align_form(const void* const feats[4], const int64_t feat_lo[4], const int32_t heights[4], const int32_t widths[4],
                         const float scales[4], int nlevels, const float* rois, int n_entries_cap, int slots_per_image, int P, int out_halo,
                         int precision, void* out, int64_t out_lo, const int32_t* slot_list, const int32_t* n_entries,
                         const int32_t* per_image_count, const int32_t* order, int32_t* levels_out, void* stream);
int rs_op_roi_align_bwd_form(float* const dfeats[4], const int32_t heights[4], const int32_t widths[4], const float scales[4], int nlevels,
                             const float* rois, int n_entries_cap, int slots_per_image, int n_images, int P, int out_halo, int grad_f32,
                             const void* dout, const int32_t* slot_list, const int32_t* n_entries, const int32_t* per_image_count,
                             void* stream);

/* Training path, losses: each writes the gradient of the total loss w.r.t. its inputs (fp16, times loss_scale) and adds the
 * loss values to loss_out (fp32, for logging).  Label assignment / sampling happen before (oracle/train_oracle.py restates
 * them; their kernels are the next step).
 *  rs_op_rpn_loss : RPN.losses for ONE feature level.  head/dhead: [n][hw][cs] ([0,A) logits, [A,5A) deltas); labels:
 *                   [n][total_anchors] in {1,0,-1} after subsampling; anchors [total_anchors][4]; matched_gt
 *                   [n][total_anchors][4]; this level's anchors start at level_off.  loss_out[0] += loss_rpn_cls,
 *                   loss_out[1] += loss_rpn_loc, both / normalizer (= RPN.BATCH_SIZE_PER_IMAGE * n, R:223).
 *  rs_op_box_loss : FastRCNNOutputLayers.losses.  pred/dpred [n_rois][cs] ([0,K] logits, K = background, then 4K deltas);
 *                   gt_classes in {0..K, -1 = empty slot}; n_valid = number of sampled RoIs.  loss_out[0] += loss_cls,
 *                   loss_out[1] += loss_box_reg.
 *  rs_op_mask_loss: mask_rcnn_loss.  logits/dlogits [n_masks][side*side][cs], targets [n_masks][side*side] 0/1.
 *  rs_op_sgd_momentum: one torch.optim.SGD step on a flat fp32 tensor (grad is divided by the loss scale first).
 *  rs_op_fold_weights: fp32 master weight [cout][kpad] -> fp16 forward weight (same layout, optional per-channel scale
 *                   folded) and its transposed, tap-flipped copy [cin][kpad_t] for rs_op_conv2d_dgrad (w_bwd may be NULL). */
/* Training path, label assignment.
 *  rs_op_match    : Matcher on pairwise IoU ([EXT d2: modeling/matcher.py, structures/boxes.py]).  boxes: [n_boxes][4] shared
 *                   by all images (anchors) or [n_images][n_boxes][4] (per_image_boxes = 1, box_count[n] valid rows);
 *                   gt [n_images][gt_cap][4] (gt_cap <= 256).  matched: index of the best gt (lowest index on ties);
 *                   labels: lbl_lo / lbl_mid / lbl_hi for best IoU < t_lo / in [t_lo, t_hi) / >= t_hi (RPN: 0,-1,1 at
 *                   0.3/0.7, R:237-243; ROI heads: 0,1,1 at 0.5/0.5, R:184-188); allow_low_quality: boxes whose IoU with a
 *                   gt equals that gt's highest IoU become 1 (RPN only).
 *  rs_op_subsample: subsample_labels ([EXT d2: modeling/sampling.py]).  Positives: label != -1 && != bg_label.  rpn_mode 1
 *                   rewrites labels in place (1 / 0 / -1); otherwise `sampled` [n_images][num_samples] receives the sampled
 *                   indices (positives first, ascending inside each group, -1 padded).  The random choice is a keyed hash of
 *                   (seed, image, index): deterministic for a seed, a different uniform sample per seed. */
int rs_op_match(const float* boxes, int per_image_boxes, const int32_t* box_count, const float* gt, const int32_t* gt_count,
                int32_t* matched, int32_t* labels, float* best_iou, int n_images, int n_boxes, int gt_cap, float t_lo, float t_hi,
                int lbl_lo, int lbl_mid, int lbl_hi, int allow_low_quality, void* stream);
int rs_op_subsample(int32_t* labels, int32_t* sampled, int32_t* sampled_count, int n_images, int n, int num_samples,
                    float positive_fraction, int bg_label, int rpn_mode, uint32_t seed, void* stream);
int rs_op_rpn_loss(const float* head, void* dhead, const int32_t* labels, const float* anchors, const float* matched_gt,
                   float* loss_out, int n, int hw, int num_anchors, int cs, int level_off, int total_anchors, float normalizer,
                   float loss_scale, void* stream);
int rs_op_box_loss(const float* pred, void* dpred, const int32_t* gt_classes, const float* proposals, const float* gt_boxes,
                   float* loss_out, int n_rois, int num_classes, int cs, float n_valid, const float reg_weights[4], float loss_scale,
                   void* stream);
int rs_op_mask_loss(const float* logits, void* dlogits, const uint8_t* targets, const int32_t* gt_classes, float* loss_out, int n_masks,
                    int side, int cs, float loss_scale, void* stream);
int rs_op_sgd_momentum(float* w, float* momentum_buf, const float* grad, int64_t n, float lr, float momentum, float weight_decay,
                       float inv_loss_scale, int first_step, void* stream);
int rs_op_fold_weights(const float* w32, const float* scale, void* w_fwd, void* w_bwd, int cout, int cin, int kh, int kw, int kpad,
                       int kpad_t, void* stream);

/* The optimiser step over a table of parameter tensors: detectron2 0.6's gradient clipping, Nesterov momentum and the bias groups of
 * get_default_optimizer_params ([EXT d2: solver/build.py; torch/optim/sgd.py; torch/nn/utils/clip_grad.py]).  csrc/sgd_rule.h holds
 * the per-element rule:
 *     g = grad * inv_scale;  g = clip(g);  g += wd_seg * w;  b = mu * buf + g;  d = nesterov ? g + mu * b : b;  w -= lr_seg * d;  buf = b
 * with lr_seg = lr * bias_lr_factor and wd_seg = weight_decay_bias (where has_weight_decay_bias) on a segment flagged as a bias, lr and
 * weight_decay elsewhere.  clip_type: 0 none; 1 value, g clamped to +-clip_value; 2 norm, every tensor multiplied by its own
 * c = min(1, clip_value / (norm + 1e-6)) in fp32 as torch.nn.utils.clip_grad_norm_ forms it; 3 full_model, one c from the norm over
 * all tensors (not in detectron2 0.6's core: its DETR and Mask2Former projects add it).  norm_type: 2.0 or +inf (the largest
 * magnitude), read by types 2 and 3.  Clipping acts on grad * inv_scale: the unscaled gradient, averaged over the ranks.  A norm is
 * summed in float64 in a fixed order, rounded to fp32, then sqrtf; nothing goes through a float atomic, so two runs give the same bits,
 * and nothing is read back by the host.  With clip_type 0, no Nesterov and factor 1 the result equals rs_op_sgd_momentum's bit for bit. */
typedef struct rs_solver {
  int32_t struct_size;            /* sizeof(rs_solver), ABI check */
  int32_t nesterov;               /* 0 / 1 (SOLVER.NESTEROV); needs momentum > 0 */
  float bias_lr_factor;           /* SOLVER.BIAS_LR_FACTOR, >= 0 */
  float weight_decay_bias;        /* SOLVER.WEIGHT_DECAY_BIAS, >= 0; read when has_weight_decay_bias */
  int32_t has_weight_decay_bias;  /* 0: biases decay as the weights do */
  int32_t clip_type;              /* 0 none, 1 value, 2 norm, 3 full_model (SOLVER.CLIP_GRADIENTS.ENABLED / CLIP_TYPE) */
  float clip_value;               /* SOLVER.CLIP_GRADIENTS.CLIP_VALUE, > 0 when clip_type != 0 */
  float norm_type;                /* SOLVER.CLIP_GRADIENTS.NORM_TYPE: 2.0 or +inf, when clip_type is 2 or 3 */
} rs_solver;
/* One such step on caller-owned device buffers w / momentum_buf / grad of n floats (16-byte aligned).  The table is HOST memory:
 * segment i holds seg_count[i] >= 1 values at seg_off[i], a multiple of 4; ascending, no overlap, inside [0, n); seg_flags[i] 0 = weight,
 * 1 = bias.  Values in no segment take lr, weight_decay and no clipping.  skip (optional, device): when *skip != 0 nothing is written
 * to w or momentum_buf.  norms_out / coef_out (optional, device, fp32 [n_seg]): every segment's norm and coefficient, written by types 2
 * and 3 only.  RS_ERR_ARG, before anything is touched and with the entry's name in the text: a null pointer, a table that breaks one of
 * the rules above, a solver rs_trainer_set_solver would refuse, Nesterov with momentum <= 0.  Enqueues on `stream`; returns after its
 * scratch is released (it waits for the stream).  rs_host_sgd_segments: the same arguments as host pointers, no device; norms in plain
 * float64 order. */
int rs_op_sgd_segments(float* w, float* momentum_buf, const float* grad, int64_t n, const int64_t* seg_off, const int64_t* seg_count,
                       const int32_t* seg_flags, int n_seg, float lr, float momentum, float weight_decay, float inv_scale,
                       const rs_solver* solver, const int32_t* skip, float* norms_out, float* coef_out, void* stream);
int rs_host_sgd_segments(float* w, float* momentum_buf, const float* grad, int64_t n, const int64_t* seg_off, const int64_t* seg_count,
                         const int32_t* seg_flags, int n_seg, float lr, float momentum, float weight_decay, float inv_scale,
                         const rs_solver* solver, const int32_t* skip, float* norms_out, float* coef_out);

/* Training diagnostics of detectron2 0.6 as INTEGER counts (csrc/train_stats.h holds the per-element rules; the ratios are the
 * caller's, in double).  The three operators take device pointers, enqueue on `stream` and do not wait; the three host entries take
 * the same arguments as host pointers and need no device.  All six ADD into the counts (zero them first), and refuse, before
 * anything is touched and with their own name in the error text: null pointers (the two optional ones excepted), negative counts,
 * num_classes outside 1..8, 5 * num_classes + 1 > cs, side < 1, cs < 1 (RS_ERR_ARG); a label count or n_masks * side * side of 2^31 or
 * more (RS_ERR_UNSUPPORTED).  Sums that would pass 2^31 - 1 are the caller's to avoid.
 *  label counts: labels[count]; counts2 += {labels equal to 1, labels equal to 0}  (RPN.losses: num_pos_anchors, num_neg_anchors).
 *  box stats   : pred [n_rois][cs] (columns [0, K] are the class logits, K = background; the deltas behind are not read),
 *                gt_classes [n_rois].  A row counts when 0 <= class <= K.  Its prediction is the FIRST largest of the K + 1 logits
 *                (torch.argmax; -0.0 equals +0.0).  counts7 += {fg, bg, inst, correct, fgn, fg_correct, fg_as_bg}: fg / bg are the sums
 *                of sampled_counts [n_images][2] (nothing when it is NULL), inst the rows that count, correct those predicted as
 *                their class, fgn those with class < K, fg_correct / fg_as_bg the foreground rows predicted as their class / as K
 *                (FastRCNNOutputLayers' _log_classification_stats).
 *  mask stats  : logits [n_masks][side*side][cs], targets [n_masks][side*side], gt_classes [n_masks]; the first
 *                min(*n_masks_ptr, n_masks) entries (all n_masks when the pointer is NULL), an entry with a class outside [0, cs)
 *                skipped.  Per pixel p = logit of the entry's class > 0 (as IEEE: true for the smallest positive denormal and +inf,
 *                false for both zeros), g = target != 0.  counts5 += {pixels, p != g, g, p & !g, !p & g} (mask_rcnn_loss). */
int rs_op_label_counts(const int32_t* labels, int64_t count, int32_t* counts2, void* stream);
int rs_op_box_stats(const float* pred, const int32_t* gt_classes, int n_rois, int num_classes, int cs, const int32_t* sampled_counts,
                    int n_images, int32_t* counts7, void* stream);
int rs_op_mask_stats(const float* logits, const uint8_t* targets, const int32_t* gt_classes, const int32_t* n_masks_ptr, int n_masks,
                     int side, int cs, int32_t* counts5, void* stream);
int rs_host_label_counts(const int32_t* labels, int64_t count, int32_t* counts2);
int rs_host_box_stats(const float* pred, const int32_t* gt_classes, int n_rois, int num_classes, int cs, const int32_t* sampled_counts,
                      int n_images, int32_t* counts7);
int rs_host_mask_stats(const float* logits, const uint8_t* targets, const int32_t* gt_classes, const int32_t* n_masks_ptr, int n_masks,
                       int side, int cs, int32_t* counts5);

/* ------------------------------------------------------------------ training engine
 * Owns a forward engine (same blob, packed with train=True: fp32 master weights `<layer>.m32`, FrozenBN scales `<layer>.s`),
 * one flat fp32 master / gradient / momentum buffer in the forward GEMM layout, a gradient buffer per activation, and the
 * backward stage list.  One step = rs_trainer_set_targets, rs_trainer_forward_trunk (preprocess .. FPN), rs_trainer_rpn_forward,
 * rs_trainer_roi_step (box head: sampling, losses, backward), rs_trainer_mask_forward / _mask_backward, rs_trainer_rpn_step
 * (RPN losses + backward), rs_trainer_backward_trunk (FPN + res5..res3 from the gradients of p2..p6), rs_trainer_apply_sgd
 * (torch.optim.SGD step on every trainable tensor + refold of the fp16 operands): what detectron2 reaches through autograd +
 * SimpleTrainer.run_step
 * ([EXT d2: engine/train_loop.py]).  Tensors: "d:<forward tensor>" activation gradients (fp16, times loss_scale),
 * "g:<layer>.w|.b" gradients and "m:<layer>.w|.b" master weights (fp32, forward layout).
 * rs_spec.precision selects the arithmetic of the whole step: 1 = REFERENCE PRECISION -- activations, activation gradients and GEMM
 * operands fp32 on v_mfma_f32_16x16x4_f32 (what detectron2's SimpleTrainer computes for the reference's YAML, which has no SOLVER.AMP
 * key, R:config/detectron2_config_3bands.yaml:268-305; "d:" tensors are then fp32, blob packed with the `.w32` operands, loss_scale 1);
 * 0 = fp16 operands with fp32 master weights and a loss scale (AMPTrainer's place). */
typedef struct rs_trainer rs_trainer;
int rs_trainer_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int batch, int tile_h,
                      int tile_w, int tile_c, float loss_scale, rs_trainer** out);
/* Creation-time options of a trainer (they change its graph).  freeze_at = MODEL.BACKBONE.FREEZE_AT: 2 (rs_trainer_create's value)
 * freezes the stem and res2; 1 trains res2 as well (its blocks unfused in the forward engine, weight gradients of every res2 layer,
 * gradient group "res2"); 0 also trains the stem convolution (unfused stem.conv1 + stem.maxpool in the forward engine, input
 * gradients of res2.0 into "d:stem", then the stages bwd.stem.maxpool and bwd.stem.conv1.w, gradient group "stem").  The blob must
 * carry the `.m32` / `.s` entries of the layers trained (weights.train_tensors with the same freeze_at).  Any other value:
 * RS_ERR_UNSUPPORTED, the message names MODEL.BACKBONE.FREEZE_AT.  The new groups finish after "res3", in the order res2, stem
 * (rs_trainer_bucket_info); in the flat buffers they lie in front of res3.  opts null = the defaults. */
typedef struct rs_train_options {
  int32_t struct_size;            /* sizeof(rs_train_options), ABI check */
  int32_t freeze_at;
} rs_train_options;
int rs_trainer_create2(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int batch, int tile_h,
                       int tile_w, int tile_c, float loss_scale, const rs_train_options* opts, rs_trainer** out);
int rs_trainer_freeze_at(rs_trainer* t);
void rs_trainer_destroy(rs_trainer* t);
rs_engine* rs_trainer_engine(rs_trainer* t);
int rs_trainer_forward_trunk(rs_trainer* t, const uint8_t* tiles_dev, int n);
int rs_trainer_backward_trunk(rs_trainer* t, int n);
/* Batches of mixed sizes (INPUT.MIN_SIZE_TRAIN with MIN_SIZE_TRAIN_SAMPLING "choice" drawn per image,
 * R:config/detectron2_config_3bands.yaml:31-38; [EXT d2: data/dataset_mapper.py + structures/image_list.py ImageList.from_tensors]):
 * image i of the coming batches is resized to new_h[i] x new_w[i] (<= the trainer's network-input size, which is the canvas = the
 * largest size of the batch), the canvas is zero beyond it, and its proposals are clipped to that size.  n = 0 restores one size
 * for all.  Ground truth passed to rs_trainer_set_targets is in each image's own resized pixels. */
int rs_trainer_set_image_sizes(rs_trainer* t, const int32_t* new_h, const int32_t* new_w, int n);
/* Ground truth of the batch (host pointers): boxes in network-input pixels [n][cap][4], classes [n][cap], counts [n].
 * The classes of the counted boxes are validated: one outside [0, rs_spec.num_classes) returns RS_ERR_ARG (the message names the
 * image, the box index, the class and the range) and leaves the previous targets in place.  Slots beyond gt_count[i] are ignored. */
int rs_trainer_set_targets(rs_trainer* t, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_count, int n, int cap);
/* RPN of the training forward + RPN.losses + its backward: heads on the current FPN maps, anchor Matcher (0.3/0.7, low-quality
 * matches) and subsample_labels (256 @ 0.5) keyed by `seed`, loss_rpn_cls / loss_rpn_loc into tensor "losses"[0..1], gradients of
 * the shared head accumulated over the levels, d:p2..d:p6 overwritten with the head's input gradient.  external_labels = 1 keeps
 * the caller's "rpn_labels" / "rpn_matched" (parity tests feed the oracle's sample). */
int rs_trainer_rpn_step(rs_trainer* t, int n, uint32_t seed, int external_labels);
/* Optional: the RPN's targets of the coming step (anchor Matcher + label subsampling: functions of the ground truth and the seed only) computed
 * ahead on the trainer's side stream.  Call after rs_trainer_set_targets, before rs_trainer_forward_trunk; the rs_trainer_rpn_step of the same
 * seed then only waits for them.  Same kernels and seed as inside the step: identical labels. */
int rs_trainer_rpn_targets_async(rs_trainer* t, int n, uint32_t seed);
/* RPN head forward alone (rs_trainer_rpn_step runs it itself), then the RoI box head of the training step:
 * RPN proposals in training mode (PRE_NMS_TOPK_TRAIN 2000 per level, NMS 0.7, POST_NMS_TOPK_TRAIN 1000 per image: R:245-250;
 * rs_trainer_set_rpn_topk overrides) + gt boxes (R:193), Matcher at 0.5, subsample_labels (1024 @ 0.25, R:178,192), box-head forward on the sample,
 * loss_cls / loss_box_reg into "losses"[2..3], backward of predictor/fc2/fc1 and RoIAlign into "d32:p2".."d32:p5".  Call order of a
 * full step: forward_trunk, rpn_forward, roi_step, rpn_step, backward_trunk, apply_sgd. */
int rs_trainer_rpn_forward(rs_trainer* t, int n);
int rs_trainer_roi_step(rs_trainer* t, int n, uint32_t seed);
/* Mask head of the training step (after rs_trainer_roi_step, before rs_trainer_rpn_step): forward on the sampled foreground RoIs
 * -- entry e runs over images, then over each image's sampled foreground in order ("mask_slots", "mask_total") --; then, with the
 * host-rasterised gt masks targets[n_entries][28*28] (rs_rasterize_polygons_within_box on "roi_boxes" / "roi_gt_index"),
 * mask_rcnn_loss -> "losses"[4] and the backward of predictor / deconv / 4 convs / RoIAlign into "d32:p2".."d32:p5".  detectron2
 * rasterises the polygons on the host at the same point ([EXT d2: structures/masks.py PolygonMasks.crop_and_resize]). */
int rs_trainer_mask_forward(rs_trainer* t, int n);
int rs_trainer_mask_backward(rs_trainer* t, int n, const uint8_t* targets_host, int n_entries);
/* Read-back of the RoIs sampled by the current rs_trainer_roi_step for the host-side mask targets: boxes [n][1024][4], gt index
 * [n][1024], counts [n][2] (foreground, total).  Waits for the sampling only (own copy stream, event recorded in roi_step): the
 * box head and an already enqueued rs_trainer_mask_forward keep running while the host rasterises. */
int rs_trainer_fetch_rois(rs_trainer* t, int n, float* boxes_host, int32_t* gt_index_host, int32_t* counts_host);
/* Mask targets rasterised on the device (opt-in; the host path above is untouched).  rs_trainer_set_polygons, after
 * rs_trainer_set_targets, packs the ground-truth polygons of the batch into pinned staging and uploads them on the trainer's stream
 * (no host wait): the flat layout of rs_rasterize_entries -- polygon q = poly_len[q] doubles at polys + poly_off[q], instance g owns
 * polygons inst_first[g] .. inst_first[g+1]-1 -- plus image_first[n + 1], the first instance of every image (gt j of image i is
 * instance image_first[i] + j); coordinates in network-input pixels.  The device pool holds, for a trainer of batch capacity N, at
 * most N * 512 polygons and N * 65536 doubles (32768 vertices per image on average): a batch beyond it returns
 * RS_POLYGONS_DO_NOT_FIT (positive, not an error: nothing was copied, the trainer is as before, run this step through
 * rs_trainer_fetch_rois + rs_trainer_mask_backward).  rs_trainer_mask_backward_device replaces rs_trainer_mask_backward: it
 * rasterises entry e (the order of "mask_slots") from "roi_boxes" / "roi_gt_index" into the tensor "mask_targets" [N*256][28][28]
 * on the chain stream -- the same bytes the host path uploads; a gt index outside the image's instances gives an all-zero mask --
 * and runs the loss and the backward, with no read-back, host wait or upload.  RS_ERR_ARG when no polygons were set since the last
 * rs_trainer_set_targets.  The stage "mask.targets" is listed by rs_trainer_stage_info once the pool exists. */
#define RS_POLYGONS_DO_NOT_FIT 1
int rs_trainer_set_polygons(rs_trainer* t, const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first,
                            const int32_t* image_first, int n);
int rs_trainer_mask_backward_device(rs_trainer* t, int n);
int rs_trainer_set_rpn_topk(rs_trainer* t, int pre_nms_topk_train, int post_nms_topk_train);
/* Sampler sizes (defaults = the reference YAML: 256 @ 0.5 anchors, 1024 @ 0.25 RoIs per image). */
int rs_trainer_set_sampling(rs_trainer* t, int rpn_batch, float rpn_positive_fraction, int roi_batch, float roi_positive_fraction);
/* Weight-gradient product of the reference-precision (fp32) trainer: 0 = fp32 matrix cores (default), 1 = split operands on the fp16
 * matrix cores (rs_op_conv2d_wgrad_split; storage, forward and input gradients stay fp32).  Read when a stage launches, so it may be
 * switched between steps; the plane scratch (largest fp32 dY + largest fp32 X of one layer) is allocated when mode 1 is first set.  The
 * abs-max and split passes run inside the `*.w` stages, so rs_trainer_stage_info includes their time.  Call it between steps from the
 * thread that drives the trainer, with the trainer's device current: the first switch to mode 1 allocates on the current device and
 * waits for the trainer's stream; a failed allocation leaves the mode as it was.  RS_ERR_UNSUPPORTED on an fp16 trainer, RS_ERR_ARG on a
 * null handle or another mode. */
int rs_trainer_set_wgrad_mode(rs_trainer* t, int mode);
/* Input-gradient product dX = dY * W^T of the reference-precision (fp32) trainer: 0 = fp32 matrix cores (default), 1 = split operands on
 * the fp16 matrix cores (rs_op_conv2d_dgrad_split) for every `*.x` stage whose shape rs_op_conv2d_dgrad_split_serves accepts -- all of
 * this model's; storage, forward, losses, addends and weight gradients do not change.  The mask deconvolution's input gradient and
 * RoIAlign backward stay fp32.  Read when a stage launches.  The first switch to mode 1 allocates, on the current device, the dY plane
 * scratch of the chain stream (separate from the weight-gradient mode's) and the planes + inverse row scales of every stage's W^T;
 * every switch to mode 1 splits the current W^T, and while the mode is on every fold (rs_trainer_apply_sgd, rs_trainer_copy_state)
 * splits again.  The abs-max and plane passes run inside the `*.x` stages, so rs_trainer_stage_info includes them.
 * rs_trainer_copy_state carries the mode to the destination.  RS_ERR_UNSUPPORTED on an fp16 trainer, RS_ERR_ARG on a null handle or
 * another mode. */
int rs_trainer_set_dgrad_mode(rs_trainer* t, int mode);
/* Forward product Y = X * W of the reference-precision (fp32) trainer: 0 = fp32 matrix cores (default), 1 = split operands on the fp16
 * matrix cores (rs_op_conv2d_fwd_split) for every forward convolution / linear stage whose shape rs_op_conv2d_fwd_split_serves accepts:
 * res2..res5, the FPN, the RPN conv and heads, the box head and predictor, the mask convolutions and predictor.  The stem and the mask
 * deconvolution stay fp32.  Storage stays fp32 (the activations the ReLU masks and the weight gradients read), and the losses, both
 * backward products, the SGD step, the stage names and rs_trainer_stage_info's list do not change; the abs-max and plane passes run
 * inside the forward stages.  Read when a stage launches.  The mode lives in the trainer's forward engine, so validation inference
 * through rs_trainer_engine follows it.  The first switch to mode 1 allocates, on the current device, the X plane scratch of the chain
 * stream (sized to the largest forward input) and the planes + inverse row scales of every served layer's weight; every switch to
 * mode 1 splits every current weight, and while the mode is on every fold (rs_trainer_apply_sgd, rs_trainer_copy_state) splits the
 * trainable layers again (the frozen res2 only at switch-on).  rs_trainer_copy_state carries the mode to the destination.
 * RS_ERR_UNSUPPORTED on an fp16 trainer, RS_ERR_ARG on a null handle or another mode. */
int rs_trainer_set_fwd_mode(rs_trainer* t, int mode);
/* Training diagnostics of the step, counted on the device (opt-in, both precisions; off by default, and a trainer that never
 * switches them on keeps its stage list and tensor table).  on = 1: three counting stages run on the chain stream behind the loss
 * stages -- "box.stats" behind box.loss, "mask.stats" behind mask.loss (both mask backward entries), "rpn.stats" behind the RPN
 * losses, where the labels are final -- and add into the tensor "train_stats", int32 [16], which is zeroed wherever "losses" is:
 *   [0..1] pos, neg anchors   [2..3] fg, bg sampled RoIs   [4..8] inst, correct, fgn, fg_correct, fg_as_bg
 *   [9..13] pixels, incorrect, positive, false_pos, false_neg   [14] images of the step   [15] 0
 * with the operators' definitions above.  The tensor is allocated by the first switch-on and read by name through
 * rs_trainer_tensor (it is not enumerated); the stages are listed by rs_trainer_stage_info, last, once switched on.  Losses and
 * gradients do not change by a bit.  Read when a step runs, so it may be switched between steps; rs_trainer_copy_state does not
 * carry it.  RS_ERR_ARG on a null handle or another value, RS_ERR_UNSUPPORTED on a trainer whose capacities would let a count
 * reach 2^31. */
int rs_trainer_set_train_stats(rs_trainer* t, int on);
/* SGD with momentum on the flat buffers + refold.  The gradient is first checked for inf / nan (fp16 loss scale too large for
 * this batch): then the step is skipped on the device -- weights and momentum unchanged -- and the tensor "grad_overflow" [1]
 * reads 1; lower the scale with rs_trainer_set_loss_scale before the next forward (GradScaler semantics, no host sync here). */
int rs_trainer_apply_sgd(rs_trainer* t, float lr, float momentum, float weight_decay);
/* The solver of the following rs_trainer_apply_sgd calls (rs_solver above; opt-in, both precisions).  A trainer whose solver was never
 * set runs exactly the two launches described above, and its stage list and tensor table do not change.  The first call cuts the flat
 * buffers along the segment table below, uploads the chunk table and registers the tensors "grad_norms" and "clip_coef" (fp32
 * [segments], enumerated by rs_trainer_tensor_name); from then on rs_trainer_apply_sgd runs the segmented step: for clip types 2 and
 * 3 grad_norm_partial_kernel (which also raises "grad_overflow", replacing the separate check) + grad_norm_finish_kernel, then
 * sgd_segments_kernel.  "grad_norms" / "clip_coef" hold the last such step's values (all 0 / unwritten for types 0 and 1).  A solver
 * of all defaults (clip_type 0, no Nesterov, factor 1, no bias decay) leaves master weights and momentum bit-identical to a trainer
 * never set.  SOLVER.WEIGHT_DECAY_NORM has no counterpart: every norm layer of this model is a FrozenBN without trainable values.
 * RS_ERR_ARG on a null handle or solver, a struct_size mismatch, nesterov outside 0 / 1, a negative or non-finite bias_lr_factor or
 * weight_decay_bias, clip_type outside 0..3, clip_value <= 0 with a clip_type other than 0, norm_type other than 2 or +inf with clip
 * types 2 / 3.  Nesterov needs momentum > 0, which arrives with rs_trainer_apply_sgd: that call then returns RS_ERR_ARG before anything
 * is launched.  rs_trainer_copy_state carries the solver to the destination.  Call it between steps from the thread that drives the
 * trainer; the first call allocates on the current device and waits for the trainer's stream.
 * Segment table: the trainable tensors in buffer order, "<layer>.w" = the [Cout][Kpad] block of "g:<layer>.w" (its padding columns
 * hold an exactly zero gradient, so they do not change a norm) and "<layer>.b" = the Cout real values of the bias (not its 64-rounded
 * slot).  rs_trainer_segment_info: offset / count in floats of the flat buffers, is_bias 0 / 1; valid without a solver. */
int rs_trainer_set_solver(rs_trainer* t, const rs_solver* solver);
int rs_trainer_segment_count(rs_trainer* t);
int rs_trainer_segment_info(rs_trainer* t, int i, char* name_out /* >= 96 bytes */, int64_t* offset, int64_t* count, int* is_bias);
int rs_trainer_set_loss_scale(rs_trainer* t, float loss_scale);
int rs_trainer_sync(rs_trainer* t);
int rs_trainer_tensor(rs_trainer* t, const char* name, void** dev_ptr, int* dtype, int* ndim, int64_t dims[5], int* halo);
int rs_trainer_tensor_count(rs_trainer* t);
int rs_trainer_tensor_name(rs_trainer* t, int i, char* name_out);
/* Multi-scale training (INPUT.MIN_SIZE_TRAIN sampling "choice", R:31-38): build one trainer per network-input size (same
 * weights, spec.min_size_test = that size) and, when the size of the next batch differs from the previous one's, carry the
 * optimiser state over: master weights + momentum are copied device to device and dst's fp16 operands refolded.  Trainers whose
 * freeze_at differ have different parameter layouts and are refused (RS_ERR_ARG).  The solver (rs_trainer_set_solver) travels with
 * the state: dst takes src's, or goes back to the plain step when src never had one. */
int rs_trainer_copy_state(rs_trainer* dst, rs_trainer* src);
/* Data parallel: every rank all-reduces (SUM) the flat gradient buffer (rs_trainer_grad_buffer, rs_trainer_param_count floats,
 * device memory) and sets the divisor to the world size, which rs_trainer_apply_sgd applies together with the loss scale
 * (DistributedDataParallel's gradient averaging: [EXT d2: engine/defaults.py create_ddp_model]). */
int rs_trainer_set_grad_divisor(rs_trainer* t, float divisor);
void* rs_trainer_master_buffer(rs_trainer* t);
int64_t rs_trainer_param_count(rs_trainer* t);
void* rs_trainer_grad_buffer(rs_trainer* t);
/* Bucketed, overlapped gradient all-reduce (what DistributedDataParallel's bucketing does with autograd hooks).  The flat
 * gradient buffer is cut into contiguous buckets listed in the order a step COMPLETES them: "heads" (box / mask / RPN heads,
 * complete after rs_trainer_rpn_step), "fpn", "res5", "res4", "res3" (completed one after the other inside
 * rs_trainer_backward_trunk).  rs_trainer_bucket_info: offset / count in floats from rs_trainer_grad_buffer.
 * rs_trainer_bucket_wait(i, stream): work enqueued on `stream` afterwards (the collective of bucket i) runs behind the
 * kernels that produce bucket i's gradients of the step enqueued so far -- a device-side wait, the caller does not block, so
 * bucket i's all-reduce overlaps the rest of the backward pass.  rs_trainer_bucket_sync(i): the host-side form (collectives
 * through host memory).  rs_trainer_wait_stream(stream): the trainer's own stream waits for everything enqueued on `stream` so
 * far; call it after the last collective and before rs_trainer_apply_sgd. */
/* Per-stage timing of the training step (bench.py --train): HIP events around every stage -- the forward stages of the training
 * step, then the box / mask / RPN / trunk backward lists -- on the stream the stage runs on, no host wait.  on = 1 clears the
 * accumulators and starts; rs_trainer_stage_count() resolves what has been recorded (it synchronises the trainer's streams).
 * flops = algorithmic FLOP of the stage's last execution (0 for non-GEMM stages); on_side_stream = 1 for weight / bias gradients
 * and RoIAlign backward, which run next to the input-gradient chain. */
int rs_trainer_set_profiling(rs_trainer* t, int on);
int rs_trainer_stage_count(rs_trainer* t);
int rs_trainer_stage_info(rs_trainer* t, int i, char* name_out /* >= 96 bytes */, double* ms_total, int* calls, double* flops, int* on_side_stream);
int rs_trainer_bucket_count(rs_trainer* t);
int rs_trainer_bucket_info(rs_trainer* t, int i, char* name_out /* >= 96 bytes */, int64_t* offset, int64_t* count);
int rs_trainer_bucket_wait(rs_trainer* t, int i, void* stream);
int rs_trainer_bucket_sync(rs_trainer* t, int i);
int rs_trainer_wait_stream(rs_trainer* t, void* stream);

/* -------- host-only helpers (no GPU needed) -------- */
/* detectron2 ResizeShortestEdge.get_output_shape. */
void rs_resize_shape(int h, int w, int short_edge, int max_size, int* new_h, int* new_w);
/* Pillow bilinear coefficient tables for in_size -> out_size: bounds[out][2] = (first, count),
 * coeffs[out][ksize] 22-bit fixed point.  Returns ksize; pass NULL pointers to query it. */
int rs_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coeffs);

int rs_memcpy_d2h(void* dst_host, const void* src_dev, size_t nbytes);
/* out[i] = a[i] / b[i] (device pointers) through csrc/common.h rs_fdiv, the division every kernel of the library uses instead of the compiler's
 * v_div_scale / v_div_fmas / v_div_fixup sequence; exported for its test. */
int rs_op_fdiv(const float* a, const float* b, float* out, int64_t n, void* stream);
int rs_memcpy_h2d(void* dst_dev, const void* src_host, size_t nbytes);
const char* rs_last_error(void);
int rs_abi_version(void);

/* Weight blob: little-endian; header {u32 magic 'RSEW', u32 version, u32 n, u32 data_offset};
 * n entries {char name[96]; u32 dtype; u32 ndim; u64 dims[4]; u64 offset; u64 nbytes}; data
 * 256-byte aligned.  Entries "<layer>.w" (fp16 [Cout_pad][Kpad], FrozenBN folded) and
 * "<layer>.b" (fp32) for every conv/linear layer, detectron2 layer names. */

/* ------------------------------------------------------------------ detections -> polygons (host code)
 * What the object-detector's detectron2dets_to_features does per instance after the predictor returns
 * ([EXT od: helpers/detectron2.py]; R:config/config_obj_detec.yaml:87-89): rasterio.features.shapes on the
 * instance mask (4-connected regions, rings along pixel edges, holes) and Ramer-Douglas-Peucker (epsilon in
 * pixels; <= 0 disables).  masks = rs_dets.masks layout, [n][h][(w+7)/8] bit-packed LSB first.  Instances are
 * spread over `threads` host threads (0 = all cores).  The result is a flat ragged structure:
 *   inst_poly_count[n]      polygons of every instance
 *   poly_ring_count[np]     rings of every polygon (exterior first, then holes)
 *   ring_len[nr]            vertices of every ring (closed: first == last)
 *   xy[2*nv]                pixel-corner coordinates (x = column, y = row), float64
 * Python restatement with identical vertex output: proj_roadsurf_amd/vectorize.py. */
typedef struct rs_vec_result rs_vec_result;
rs_vec_result* rs_vectorize_masks(const uint8_t* masks, int n, int h, int w, double rdp_epsilon, int threads);
/* The same for masks that arrive as crops (rs_mask_crops): rects [n][4], offsets [n] into data. */
rs_vec_result* rs_vectorize_mask_crops(const uint8_t* data, const int32_t* rects, const uint32_t* offsets, int n, int h, int w,
                                       double rdp_epsilon, int threads);
void rs_vec_counts(const rs_vec_result* r, int64_t* n_instances, int64_t* n_polygons, int64_t* n_rings, int64_t* n_vertices);
int rs_vec_copy(const rs_vec_result* r, int32_t* inst_poly_count, int32_t* poly_ring_count, int32_t* ring_len, double* xy);
void rs_vec_free(rs_vec_result* r);
/* GeoPackage geometry blobs ('GP' header + little-endian WKB Polygon, OGC 12-128r15) of every polygon of a result, coordinates
 * georeferenced per instance: X = xform[i][0] + x*xform[i][2], Y = xform[i][1] - y*xform[i][3] (xform NULL = pixel coordinates,
 * Y = y) -- what the reference writes through geopandas.to_file(driver="GPKG") (R:config/config_obj_detec.yaml:100-103).
 * out NULL: returns the bytes needed; else fills out, offsets[n_polygons+1] and bbox[minx,miny,maxx,maxy]. */
int64_t rs_vec_gpkg_blobs(const rs_vec_result* r, const double* xform, int32_t srs_id, uint8_t* out, int64_t out_cap,
                          int64_t* offsets, double bbox[4]);

/* ------------------------------------------------------------------ detections -> polygons on the device (csrc/polygonize.hip)
 * The same mask -> polygon -> Ramer-Douglas-Peucker tail as rs_vectorize_masks, vertex for vertex, as HIP kernels: one workgroup per
 * instance, its working set in LDS.  An instance whose mask needs more than the per-instance capacities (directed
 * edges, rings, ring vertices before simplification: rs_polygonize_caps) is FLAGGED and produces no rows; the caller vectorises it on
 * the host (rs_vectorize_masks / rs_vectorize_mask_crops) and rs_vec_from_tables merges the two, so nothing is dropped or truncated.
 * Tables: header [n][RS_POLY_HDR] int32 = {flagged, polygons, rings, vertices, first polygon, first ring, first vertex, 0} per instance;
 * poly_ring_count / ring_len as in rs_vec_result over the instances that are not flagged, in order; xy = int16 (x, y) pairs in tile
 * pixels (integers by construction; canvases up to 1024 x 1024).  totals [4] = {polygons, rings, vertices, flagged instances}. */
#define RS_POLY_HDR 8
void rs_polygonize_caps(int* edge_cap, int* vertex_cap, int* ring_cap, int* max_side);
/* Stand-alone operator on caller-owned device memory: masks_dev [n][h][(w+7)/8]; edge_cap / vertex_cap 0 = the default (the maximum).
 * Output device buffers sized for the worst case: header n * RS_POLY_HDR, poly_ring_count and ring_len n * ring_cap each, xy n *
 * vertex_cap pairs, totals 4.  Waits for the stream. */
int rs_op_polygonize(const uint8_t* masks_dev, int n, int h, int w, double rdp_epsilon, int edge_cap, int vertex_cap, int32_t* header_dev,
                     int32_t* poly_ring_count_dev, int32_t* ring_len_dev, int16_t* xy_dev, int32_t* totals_dev, void* stream);
/* The same in the form the engine calls it: masks_dev [tiles * slots][h][(w+7)/8] canvases, instance = tile * slots + slot.
 * det_count_dev [tiles] (NULL: every slot is valid): slots at or past a tile's count give an all-zero header.  rects_dev
 * [tiles * slots][4] as rs_mask_crops.rects (NULL: whole canvases): only the rectangle is read, as a mask of its own with background
 * around it, and the vertices stay in tile pixels; a rectangle with a negative field or one that leaves the canvas flags its
 * instance.  Output buffers sized for tiles * slots instances. */
int rs_op_polygonize_crops(const uint8_t* masks_dev, int tiles, int slots, const int32_t* det_count_dev, const int32_t* rects_dev, int h, int w,
                           double rdp_epsilon, int edge_cap, int vertex_cap, int32_t* header_dev, int32_t* poly_ring_count_dev, int32_t* ring_len_dev,
                           int16_t* xy_dev, int32_t* totals_dev, void* stream);
/* Host only: an rs_vec_result over n instances from the tables above.  `fallback` holds the host-vectorised flagged instances, one
 * per flagged header in slot order (NULL when none is flagged); NULL is returned when the tables and the fallback do not fit together.
 * rs_vec_counts / rs_vec_copy / rs_vec_gpkg_blobs serve the result as any other. */
rs_vec_result* rs_vec_from_tables(const int32_t* header, int n, const int32_t* poly_ring_count, const int32_t* ring_len, const int16_t* xy,
                                  const rs_vec_result* fallback);

/* Polygons of the last forward, the counterpart of rs_engine_fetch_crops_*: caller-allocated (rs_host_alloc) tables for n tiles of D
 * slots each; poly_cap / ring_cap / vertex_cap = elements available (n * D * ring_cap, the same, n * D * vertex_cap always suffice). */
typedef struct rs_polygons {
  int32_t* header;            /* [n][D][RS_POLY_HDR] */
  int32_t* poly_ring_count;
  int32_t* ring_len;
  int16_t* xy;
  uint64_t poly_cap, ring_cap, vertex_cap;
  uint64_t n_polygons, n_rings, n_vertices, n_flagged;  /* out (rs_engine_fetch_polygons_wait) */
  rs_mask_crops* crops;       /* crop table (always filled) and data (copied only when an instance was flagged or want_masks) */
  int32_t want_masks;         /* in: copy the crop bytes in any case */
  int32_t masks_copied;       /* out: crops->data / crops->used are valid */
} rs_polygons;
/* rs_engine_fetch_polygons_async enqueues, on the copy stream behind the forward, the crop planning, the polygoniser (rdp_epsilon <= 0:
 * no simplification) and the copies of count / boxes / scores / classes, the crop table and the polygon headers;
 * rs_engine_fetch_polygons_wait waits for them, copies exactly the rows in use and -- only when an instance was flagged or masks were
 * asked for -- the crop bytes.  The engine's result buffers are free for the next forward after the first step.  MASK_ON false:
 * RS_ERR_ARG.  The device buffers are allocated on the first call. */
int rs_engine_fetch_polygons_async(rs_engine* e, int n, rs_dets* dets_host, rs_polygons* polys_host, double rdp_epsilon);
int rs_engine_fetch_polygons_wait(rs_engine* e, rs_polygons* polys_host);

/* Training targets of the mask head (host code): the polygons of ONE ground-truth instance cropped to `box` and rasterised at
 * mask_size x mask_size -- PolygonMasks.crop_and_resize ([EXT d2: structures/masks.py rasterize_polygons_within_box]; rasteriser =
 * pycocotools' rleFrPoly restated, parity unpinned).  polys: concatenated [x0,y0,x1,y1,...] of the polygons, poly_len[i] doubles
 * each; out: [mask_size][mask_size] 0/1. */
int rs_rasterize_polygons_within_box(const double* polys, const int32_t* poly_len, int n_polys, const double box[4], int mask_size,
                                     uint8_t* out);
/* The same for every sampled foreground RoI of a training step in one call (host threads over the entries; threads <= 0: up
 * to 16): instance g owns polygons inst_first[g] .. inst_first[g+1]-1, polygon q = poly_len[q] doubles at polys + poly_off[q];
 * entry e rasterises instance entry_inst[e] inside boxes[e] (x1,y1,x2,y2 as read back from "roi_boxes") -> out[e][S*S]. */
int rs_rasterize_entries(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst,
                         const int32_t* entry_inst, const float* boxes, int n_entries, int mask_size, uint8_t* out, int threads);

/* rs_rasterize_entries on the GPU (mask_targets_kernel, the kernel behind rs_trainer_mask_backward_device): same arguments (host
 * pointers) without `threads`, same bytes out.  Uploads the polygons, rasterises the n_entries (instance, box) pairs, one workgroup
 * each, and copies the masks back.  mask_size even, up to RS_MASK_SIDE.  Unlike the host call, an entry whose instance is outside
 * [0, n_inst) is not an error: its mask is all zero. */
int rs_op_mask_targets(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst,
                       const int32_t* entry_inst, const float* boxes, int n_entries, int mask_size, uint8_t* out);

/* ------------------------------------------------------------------ validation AP on the device (csrc/val_ap.hip)
 * The segm side of COCO AP needs, per (detection, ground truth) pair, the pixel count of the intersection and the two areas: integers
 * that decide the float64 IoU completely (proj_roadsurf_amd/coco_eval.py mask_iou_from_counts).
 *
 * rs_op_rasterize_canvas: the polygon tables of rs_op_mask_targets (host pointers), one instance per ground truth, rasterised onto
 * whole side x side canvases in the rs_dets.masks layout -- out [n_inst][side][(side+7)/8] bytes (host), bit x % 8 of byte x / 8 =
 * pixel x, padding bits zero -- bit for bit rs_rasterize_polygons_within_box(instance's polygons, box (0, 0, side, side), side).
 * side in [1, 1024]; an instance without polygons gives an all-zero mask.  Null tables, a side outside the range and an odd poly_len
 * are refused (RS_ERR_ARG) before a device is touched.
 *
 * rs_op_mask_pair_counts: caller-owned device memory.  det_masks [n_tiles][slots][side][(side+7)/8], det_count [n_tiles]; gt_masks
 * [instances][side][(side+7)/8] (as rs_op_rasterize_canvas writes them), tile t owning instances tile_first[t] .. tile_first[t+1]-1
 * (at most gt_cap of them are read).  Out, int32: inter [n_tiles][slots][gt_cap] = popcount(detection AND ground truth), det_area
 * [n_tiles][slots], gt_area [n_tiles][gt_cap]; slots at or past det_count[t] and ground truths past the tile's own are zero.
 * side * ((side+7)/8) must be a multiple of 4 (RS_ERR_UNSUPPORTED otherwise).  Enqueues on `stream`, does not wait. */
int rs_op_rasterize_canvas(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst,
                           int side, uint8_t* out);
int rs_op_mask_pair_counts(const uint8_t* det_masks, const int32_t* det_count, int n_tiles, int slots, const uint8_t* gt_masks,
                           const int32_t* tile_first, int gt_cap, int side, int32_t* inter, int32_t* det_area, int32_t* gt_area, void* stream);

/* The same on the detections of the engine's last forward, the counterpart of rs_engine_fetch_crops_*: rs_engine_fetch_eval_async
 * packs the ground-truth polygons of the batch's n tiles (tables as above; tile_first [n + 1], the first instance of every tile; tile
 * pixels) into pinned staging and enqueues, on the copy stream behind the forward, their upload, the rasteriser, the pair counts and
 * the copies of count / boxes / scores / classes (dets->masks and ->mask_probs are ignored: no mask travels) and of the three tables
 * into caller-allocated (rs_host_alloc) buffers inter [n][D][RS_EVAL_GT_CAP], det_area [n][D], gt_area [n][RS_EVAL_GT_CAP].
 * rs_engine_fetch_eval_wait waits for them.  The device pool holds, for an engine of max_batch N, N * RS_EVAL_GT_CAP instances with
 * at most RS_EVAL_GT_CAP per tile, N * 512 polygons and N * 65536 doubles; it is allocated on the first call.  A batch beyond it, a
 * non-square tile, a side above 1024 or one whose packed masks are no whole 32-bit words, and an engine with MASK_ON false return
 * RS_EVAL_DOES_NOT_FIT (positive, not an error: nothing was enqueued, evaluate this batch from rs_engine_fetch's masks).
 * rs_engine_eval_fits is that check alone (host only), for a caller that wants to know before the forward. */
#define RS_EVAL_DOES_NOT_FIT 2
#define RS_EVAL_GT_CAP 128
typedef struct rs_eval_counts {
  int32_t* inter;     /* [n][D][RS_EVAL_GT_CAP] */
  int32_t* det_area;  /* [n][D] */
  int32_t* gt_area;   /* [n][RS_EVAL_GT_CAP] */
} rs_eval_counts;
int rs_engine_eval_fits(rs_engine* e, int n, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, const int32_t* tile_first);
int rs_engine_fetch_eval_async(rs_engine* e, int n, rs_dets* dets_host, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                               const int32_t* inst_first, const int32_t* tile_first, rs_eval_counts* counts_host);
int rs_engine_fetch_eval_wait(rs_engine* e);

/* ------------------------------------------------------------------ COCOeval's evaluateImg on the device (csrc/coco_match.h)
 * The step after the counts: per tile, kind (0 bbox, 1 segm), area range (all, small, medium, large) and IoU threshold, the greedy
 * matching of detections to ground truths that proj_roadsurf_amd/coco_eval.py match_images runs on the host, with identical flags.
 * csrc/coco_match.h states the rule once, for the kernels (csrc/val_ap.hip) and the host restatement: box IoU in float64 in
 * coco_eval.box_iou's operation order (detection boxes are the engine's float32 values widened, ground-truth boxes float64 XYXY),
 * mask IoU from the three pixel counts, the compiler's correctly rounded float64 division, no mul+add contraction; a ground truth is
 * ignored when its area (bbox: the box's, segm: the pixel count) is < lo or > hi of the range; detections per category by descending
 * score, ties to the lower slot; a detection takes the unmatched ground truth of its category with the highest IoU >=
 * min(threshold, 1 - 1e-10), kept ones before ignored ones, of equal IoUs the LATER one; a detection matched to an ignored ground
 * truth, or unmatched with its own area outside the range, is ignored.  Crowd regions and annotated areas are not modelled (such a
 * batch is matched on the host); max_dets is the slot count.
 *
 * Tables: det_boxes [n_tiles][slots][4], det_scores / det_classes [n_tiles][slots], det_count [n_tiles] as rs_dets; gt_boxes
 * [instances][4] double, gt_classes [instances], tile t owning instances tile_first[t] .. tile_first[t+1]-1 (at most gt_cap are
 * read); inter / det_area / gt_area as rs_op_mask_pair_counts writes them; iou_thrs = ten doubles on the HOST in both entries (they
 * travel by value: coco_eval.IOU_THRS as numpy holds them, 0.8999999999999999 among them).  Out, with W = (slots + 31) / 32:
 *   order        [n_tiles][slots] int32   position -> slot, sorted by (category, score descending, slot); a class outside
 *                                         [0, num_classes) sorts behind every category; positions >= det_count hold -1
 *   class_first  [n_tiles][num_classes + 1] int32   first position of each category in `order`
 *   gt_per_class [n_tiles][num_classes] int32       ground truths per category
 *   matched, ignored [n_tiles][2][4][10][W] uint32  bit p % 32 of word p / 32 = the flag of position p; padding bits zero
 *   npig         [n_tiles][2][4][num_classes] int32 ground truths the range does not ignore
 * rs_op_coco_match takes device pointers, enqueues on `stream` and does not wait; rs_host_coco_match takes the same arguments as host
 * pointers and needs no device.  Both refuse, before anything is touched: a null table, n_tiles < 1, num_classes outside
 * [1, RS_MAX_CLASSES], slots or gt_cap < 1 (RS_ERR_ARG); slots > 1024 or gt_cap > RS_EVAL_GT_CAP (RS_ERR_UNSUPPORTED). */
int rs_op_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes, const int32_t* det_count,
                     const double* gt_boxes, const int32_t* gt_classes, const int32_t* tile_first, const int32_t* inter,
                     const int32_t* det_area, const int32_t* gt_area, const double* iou_thrs, int n_tiles, int num_classes, int slots,
                     int gt_cap, int32_t* order, int32_t* class_first, int32_t* gt_per_class, uint32_t* matched, uint32_t* ignored,
                     int32_t* npig, void* stream);
int rs_host_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes, const int32_t* det_count,
                       const double* gt_boxes, const int32_t* gt_classes, const int32_t* tile_first, const int32_t* inter,
                       const int32_t* det_area, const int32_t* gt_area, const double* iou_thrs, int n_tiles, int num_classes, int slots,
                       int gt_cap, int32_t* order, int32_t* class_first, int32_t* gt_per_class, uint32_t* matched, uint32_t* ignored,
                       int32_t* npig);

/* The same behind the engine's last forward: rs_engine_fetch_eval_match_async enqueues what rs_engine_fetch_eval_async enqueues
 * (polygon upload, rasteriser, pair counts), then the upload of the batch's ground-truth boxes and classes (gt_boxes [tile_first[n]][4],
 * gt_classes [tile_first[n]], host), the order pass and the match pass, and the copies of count / boxes / scores / classes and of the
 * five tables (gt_cap = RS_EVAL_GT_CAP, slots = D, num_classes = the engine's) into caller-allocated (rs_host_alloc) buffers; the
 * inter / area tables stay on the device.  The same pool, the same RS_EVAL_DOES_NOT_FIT conditions (rs_engine_eval_fits; also D >
 * 1024) and the same rule that a batch that does not fit enqueues nothing.  rs_engine_fetch_eval_match_wait waits for the copies. */
typedef struct rs_eval_matches {
  int32_t* order;         /* [n][D] */
  int32_t* class_first;   /* [n][K + 1] */
  int32_t* gt_per_class;  /* [n][K] */
  uint32_t* matched;      /* [n][2][4][10][(D + 31) / 32] */
  uint32_t* ignored;      /* [n][2][4][10][(D + 31) / 32] */
  int32_t* npig;          /* [n][2][4][K] */
} rs_eval_matches;
int rs_engine_fetch_eval_match_async(rs_engine* e, int n, rs_dets* dets_host, const double* polys, const int64_t* poly_off,
                                     const int32_t* poly_len, const int32_t* inst_first, const int32_t* tile_first, const double* gt_boxes,
                                     const int32_t* gt_classes, const double* iou_thrs, rs_eval_matches* matches_host);
int rs_engine_fetch_eval_match_wait(rs_engine* e);

/* ------------------------------------------------------------------ the road cover vote on the device (csrc/road_vote.h)
 * The project's deliverable is a cover class per road: the reference overlays the tile-clipped road labels with the detections,
 * weights every (road, detection) pair by round(area(intersection) / area(label), 2), keeps the pairs above 0.05 whose score reaches
 * a threshold and sums, per road and class, weighted scores and weights (proj_roadsurf_amd/raster_vote.py weighted_scores,
 * determine_detected_class).  A road label in tile pixels is the same object as a ground-truth instance of the validation counts, so
 * the stage runs on the tables rs_op_mask_pair_counts writes, one label per "ground truth".  Areas are whole pixels of the tile grid
 * and polygon simplification does not enter.  csrc/road_vote.h states the rule once, for the kernel (csrc/val_ap.hip) and the host
 * restatement: for every tile t, label g < min(tile_first[t+1] - tile_first[t], gt_cap) with A = gt_area[t][g] > 0 and class c, the
 * slots d = 0 .. det_count[t] - 1 in ascending order; with I = inter[t][d][g] > 0 and det_classes[t][d] == c,
 * frac = rint((double)I / (double)A * 100.0) / 100.0 (numpy's round(I / A, 2)); a pair with frac > 0.05 and (double)score >=
 * threshold adds frac * (double)score to wscore, frac to wfrac and 1 to pairs.  float64, the compiler's correctly rounded division,
 * no mul+add contraction, no atomics: the bits do not depend on the run.
 *
 * Tables: det_scores / det_classes [n_tiles][slots], det_count [n_tiles] as rs_dets; tile_first [n_tiles + 1]; inter
 * [n_tiles][slots][gt_cap] and gt_area [n_tiles][gt_cap] as rs_op_mask_pair_counts writes them.  Out: wscore, wfrac
 * [n_tiles][gt_cap][num_classes] double, pairs [n_tiles][gt_cap][num_classes] int32; rows of labels past the tile's own and of
 * labels with area 0 are zero, a detection whose class lies outside [0, num_classes) votes for nothing.
 * rs_op_road_votes takes device pointers, clears its outputs, enqueues on `stream` and does not wait; rs_host_road_votes takes the
 * same arguments as host pointers and needs no device.  Both refuse, before anything is touched: a null table, n_tiles < 1,
 * num_classes outside [1, RS_MAX_CLASSES], slots or gt_cap < 1, a threshold that is not finite (RS_ERR_ARG); slots > 1024 or gt_cap
 * > RS_EVAL_GT_CAP (RS_ERR_UNSUPPORTED). */
int rs_op_road_votes(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                     const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap, double threshold,
                     double* wscore, double* wfrac, int32_t* pairs, void* stream);
int rs_host_road_votes(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                       const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap, double threshold,
                       double* wscore, double* wfrac, int32_t* pairs);

/* The same behind the engine's last forward.  rs_engine_fetch_votes_async is an add-on, not a fetch form: it carries no rs_dets and
 * may follow any rs_engine_fetch*_async of the same forward (plain, crops, polygons) or stand alone.  It packs the road labels of the
 * batch's n tiles (the polygon tables of rs_engine_fetch_eval_async: one instance per label, tile pixels) and enqueues, on the copy
 * stream behind the forward and behind that fetch: their upload, the rasteriser, the pair counts, the vote (gt_cap = RS_EVAL_GT_CAP,
 * slots = D, num_classes = the engine's) and the copies of the three vote tables and of gt_area into caller-allocated
 * (rs_host_alloc) buffers.  No mask leaves the device and `inter` stays there.  It shares the pool of the validation counts and its
 * limits, and returns RS_EVAL_DOES_NOT_FIT with nothing enqueued under the conditions of rs_engine_eval_fits (also D > 1024): vote
 * on that batch from fetched masks.  The next forward on the engine is ordered behind it as behind rs_engine_fetch_eval_async.  An
 * engine that never calls it allocates nothing for it.  rs_engine_fetch_votes_wait waits for the copies (and for whatever else is
 * on the copy stream in front of them); a crops or polygons fetch in flight is still completed by its own wait. */
typedef struct rs_road_votes {
  double* wscore;       /* [n][RS_EVAL_GT_CAP][K] */
  double* wfrac;        /* [n][RS_EVAL_GT_CAP][K] */
  int32_t* pairs;       /* [n][RS_EVAL_GT_CAP][K] */
  int32_t* label_area;  /* [n][RS_EVAL_GT_CAP] */
} rs_road_votes;
int rs_engine_fetch_votes_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                const int32_t* inst_first, const int32_t* tile_first, double threshold, rs_road_votes* votes_host);
int rs_engine_fetch_votes_wait(rs_engine* e);

/* The vote for a list of score thresholds at once.  The reference's published number is the balanced F1 of the road cover classes at
 * the best of 20 thresholds (scripts/road_segmentation/final_metrics.py runs determine_detected_class once per value of
 * np.arange(0, 1., 0.05)); proj_roadsurf_amd/road_metrics.py restates its metrics on the road tables.  thresholds[0 .. n_thresholds - 1]
 * is a HOST pointer in every entry below and is copied into the launch parameters: 1 <= n_thresholds <= RS_VOTE_SWEEP_MAX, any finite
 * doubles in any order, duplicates allowed.  Out: wscore, wfrac [n_tiles][n_thresholds][gt_cap][num_classes] double and pairs of the
 * same shape int32.  Slice j has the bits of rs_op_road_votes' tables at threshold thresholds[j]: the same walk over the slots, the
 * same float64 arithmetic, once per threshold (csrc/road_vote.h, THE SWEEP; road_vote_sweep_kernel in csrc/val_ap.hip carries the
 * threshold's index in the grid, so the compare is against one value per wave).  rs_op_road_votes_sweep takes device tables, clears
 * its outputs, enqueues on `stream` and does not wait; rs_host_road_votes_sweep takes host tables and needs no device.  Both refuse,
 * before anything is touched, what the single-threshold entries refuse, and also a null list, n_thresholds outside
 * [1, RS_VOTE_SWEEP_MAX] and an entry that is not finite (RS_ERR_ARG). */
#define RS_VOTE_SWEEP_MAX 32
int rs_op_road_votes_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                           const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap,
                           const double* thresholds, int n_thresholds, double* wscore, double* wfrac, int32_t* pairs, void* stream);
int rs_host_road_votes_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                             const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap,
                             const double* thresholds, int n_thresholds, double* wscore, double* wfrac, int32_t* pairs);

/* The sweep behind the engine's last forward: an add-on exactly like rs_engine_fetch_votes_async (label upload, rasteriser, pair
 * counts, the sweep and the copies on the copy stream, behind the forward and behind any fetch of it; the same pool, the same limits,
 * RS_EVAL_DOES_NOT_FIT with nothing enqueued under the same conditions; the next forward is ordered behind it in the same way).  The
 * rasteriser and the pair counts run once for all thresholds.  The device tables are allocated on the first call, sized for
 * RS_VOTE_SWEEP_MAX thresholds; an engine that never calls it allocates nothing for it, and its stages and tensors are unchanged.
 * The caller's (rs_host_alloc) tables hold n * n_thresholds * RS_EVAL_GT_CAP * K cells each, label_area n * RS_EVAL_GT_CAP. */
typedef struct rs_road_vote_sweep {
  double* wscore;       /* [n][T][RS_EVAL_GT_CAP][K] */
  double* wfrac;        /* [n][T][RS_EVAL_GT_CAP][K] */
  int32_t* pairs;       /* [n][T][RS_EVAL_GT_CAP][K] */
  int32_t* label_area;  /* [n][RS_EVAL_GT_CAP] */
} rs_road_vote_sweep;
int rs_engine_fetch_vote_sweep_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                     const int32_t* inst_first, const int32_t* tile_first, const double* thresholds, int n_thresholds,
                                     rs_road_vote_sweep* sweep_host);
int rs_engine_fetch_vote_sweep_wait(rs_engine* e);

/* ------------------------------------------------------------------ the vote on polygon areas (csrc/poly_overlap.h)
 * An opt-in geometry of the same vote: the reference overlays the vector road labels with the POLYGONS that make_detections wrote
 * (after Ramer-Douglas-Peucker) and weights a pair by round(area(label ∩ detection) / area(label), 2), both areas on polygons.  The
 * entries below compute that weight from the device polygoniser's vertex tables and the labels' float64 rings, exactly as far as
 * float64 allows: csrc/poly_overlap.h states the closed-form sum over pairs of edges, its summation order (which the host restatement
 * repeats bit for bit), the translation, and the error bound po_bound on the computed area.  A detection's first ring per polygon is
 * its exterior, the rest are holes, an instance of several polygons is their sum.  EVERY LABEL RING IS AN EXTERIOR and a label's
 * rings are taken as simple and pairwise interior-disjoint (area(label) = the sum of |shoelace| / 2 over its rings); the pixel
 * geometry above takes the union of a label's rings instead.  This is not checked; overlapping label rings and labels with holes are
 * not covered.  Area ratios do not change under the tile's affine map, so georeferencing does not enter.
 *
 * Tables of rs_op_polygon_overlaps (device pointers, clears its outputs, enqueues on `stream`, does not wait) and
 * rs_host_polygon_overlaps (host pointers, no device): header [n_tiles * slots][RS_POLY_HDR], poly_ring_count, ring_len, xy as
 * rs_op_polygonize_crops writes them (instance = tile * slots + slot); det_count [n_tiles]; the labels as the packed pool holds
 * them: tile_first [n_tiles + 1] (first label of every tile, at most gt_cap are read), inst_first [labels + 1] (first ring of every
 * label), poly_off [rings] int32 (doubles into polys), poly_len [rings] (doubles), polys float64 tile pixels.  Out: frac
 * [n_tiles][slots][gt_cap] double (the rounded weight; 0 for pairs whose boxes do not overlap, for slots at or past det_count, for
 * labels past the tile's own or of area 0), label_area [n_tiles][gt_cap] double, flagged [n_tiles] int32 = instances among the
 * tile's slots in use that the polygoniser flagged: they have no rows, their pairs are 0, and the caller redoes such a tile on the
 * host after vectorising them there.  raw_areas != 0 leaves the last step out: `frac` then holds the computed areas A themselves,
 * which is how the tests hold them to po_bound.  Both refuse, before anything is touched, a null table, n_tiles < 1, slots or gt_cap < 1
 * (RS_ERR_ARG); slots > 1024 or gt_cap > RS_EVAL_GT_CAP (RS_ERR_UNSUPPORTED).
 *
 * rs_op_road_votes_area_sweep / rs_host_road_votes_area_sweep: rs_op_road_votes_sweep with `frac` in place of inter / gt_area -- the
 * same walk over the slots (csrc/road_vote.h, rv_pair_area: class test, frac > 0.05, score >= threshold, the three accumulators, slots
 * ascending), the same tables [n_tiles][n_thresholds][gt_cap][num_classes], the same refusals and codes.  The single vote is
 * n_thresholds = 1. */
int rs_op_polygon_overlaps(const int32_t* header, const int32_t* poly_ring_count, const int32_t* ring_len, const int16_t* xy,
                           const int32_t* det_count, const int32_t* tile_first, const int32_t* inst_first, const int32_t* poly_off,
                           const int32_t* poly_len, const double* polys, int n_tiles, int slots, int gt_cap, int raw_areas, double* frac,
                           double* label_area, int32_t* flagged, void* stream);
int rs_host_polygon_overlaps(const int32_t* header, const int32_t* poly_ring_count, const int32_t* ring_len, const int16_t* xy,
                             const int32_t* det_count, const int32_t* tile_first, const int32_t* inst_first, const int32_t* poly_off,
                             const int32_t* poly_len, const double* polys, int n_tiles, int slots, int gt_cap, int raw_areas, double* frac,
                             double* label_area, int32_t* flagged);
int rs_op_road_votes_area_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                                const double* frac, int n_tiles, int num_classes, int slots, int gt_cap, const double* thresholds,
                                int n_thresholds, double* wscore, double* wfrac, int32_t* pairs, void* stream);
int rs_host_road_votes_area_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                                  const double* frac, int n_tiles, int num_classes, int slots, int gt_cap, const double* thresholds,
                                  int n_thresholds, double* wscore, double* wfrac, int32_t* pairs);

/* The same behind the engine's last forward: an add-on like rs_engine_fetch_vote_sweep_async, which must FOLLOW an
 * rs_engine_fetch_polygons_async of the same forward and batch, because it reads the vertex tables that fetch left on the device
 * (otherwise RS_ERR_ARG, nothing enqueued).  On the copy stream it enqueues the label upload, the overlap kernel, the area sweep and
 * the copies of the three vote tables, label_area (double) and flagged.  Neither the rasteriser nor the pair counts run.  The same
 * label pool and the same RS_EVAL_DOES_NOT_FIT conditions as the other add-ons; its device tables are allocated on the first call
 * (the sweep's tables are shared with rs_engine_fetch_vote_sweep_async), an engine that never calls it allocates nothing and its
 * stages and tensors are unchanged.  A tile with flagged[t] > 0 has zero weights for the flagged instances: redo it on the host. */
typedef struct rs_road_votes_poly {
  double* wscore;       /* [n][T][RS_EVAL_GT_CAP][K] */
  double* wfrac;        /* [n][T][RS_EVAL_GT_CAP][K] */
  int32_t* pairs;       /* [n][T][RS_EVAL_GT_CAP][K] */
  double* label_area;   /* [n][RS_EVAL_GT_CAP] */
  int32_t* flagged;     /* [n] */
} rs_road_votes_poly;
int rs_engine_fetch_votes_poly_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                     const int32_t* inst_first, const int32_t* tile_first, const double* thresholds, int n_thresholds,
                                     rs_road_votes_poly* votes_host);
int rs_engine_fetch_votes_poly_wait(rs_engine* e);

/* ------------------------------------------------------------------ band histograms under the road labels (csrc/band_hist.h)
 * The reference's second answer for a road's cover is statistical: scripts/statistical_analysis collects, per road, the pixels of
 * every band under the road's polygon over all tiles the road touches, drops the nodata pixels (without a nodata value in the TIFF:
 * the pixels whose bands are all 0) and tabulates min, max, median, mean, std and count per road and band, then per cover type.
 * Every one of those is an exact function of a 256-bin histogram per (road, band), and integer histograms add exactly over tiles,
 * batches and ranks.  csrc/band_hist.h states the rule once, for the kernel (csrc/band_hist.hip) and the host restatement: for tile t,
 * label instance g in tile_first[t] .. tile_first[t+1]-1, band c < channels and value v < 256, hist[g][c][v] is the number of pixels
 * (x, y) of tile t whose bit x % 8 of byte x / 8 of row y of canvas g is set, whose bands are not all 0, and whose band c equals v.  A
 * pixel with some bands 0 and others not is counted, in bin 0 of its zero bands.  Integers only: the bits do not depend on the run.
 *
 * Tables: tiles [n_tiles][side][side][channels] uint8, interleaved; label_masks [n_inst][side][(side+7)/8] in the layout
 * rs_op_rasterize_canvas writes; tile_first [n_tiles + 1] with tile_first[n_tiles] = n_inst.  Out: hist [n_inst][channels][256]
 * uint32, compact by instance (not padded to RS_EVAL_GT_CAP); a count is at most side * side <= 2^20.
 * rs_op_band_hist takes device pointers, clears hist, enqueues on `stream` and does not wait; rs_host_band_hist takes the same
 * arguments as host pointers, is plain loops over the rule and needs no device.  Both refuse, before anything is touched: a null
 * table (label_masks and hist may be null when n_inst is 0), n_tiles < 1, n_inst < 0, side outside [1, 1024], channels outside [1, 4]
 * (RS_ERR_ARG); canvases that are not whole 32-bit words, side * ((side+7)/8) % 4 != 0 (RS_ERR_UNSUPPORTED, as
 * rs_op_mask_pair_counts).  The device entry also needs label_masks 4-byte aligned. */
int rs_op_band_hist(const uint8_t* tiles, const uint8_t* label_masks, const int32_t* tile_first, int n_tiles, int n_inst, int side,
                    int channels, uint32_t* hist, void* stream);
int rs_host_band_hist(const uint8_t* tiles, const uint8_t* label_masks, const int32_t* tile_first, int n_tiles, int n_inst, int side,
                      int channels, uint32_t* hist);

/* The same behind the engine's last forward, on the tiles that forward read.  rs_engine_fetch_band_hist_async is an add-on like
 * rs_engine_fetch_votes_async: it carries no rs_dets and may follow any rs_engine_fetch*_async of the same forward, the vote add-on,
 * or stand alone.  It packs the road labels of the batch's n tiles (the polygon tables of rs_engine_fetch_eval_async) and enqueues on
 * the copy stream, in this order: their upload, the canvas rasteriser, the histogram kernel over the engine's tile buffer, and one
 * copy of tile_first[n] * C * 256 uint32 (C = the engine's tile channels) into the caller-allocated (rs_host_alloc) out->hist, whose
 * capacity is max_batch * RS_EVAL_GT_CAP * C * 256.  No pair counts are formed.  It shares the pool of the validation counts and the
 * conditions of rs_engine_eval_fits, and returns RS_EVAL_DOES_NOT_FIT with nothing enqueued when the batch does not fit: form that
 * batch's histograms on the host (rs_host_band_hist).  An engine that never calls it allocates nothing for it.
 * The tile buffer: the kernel reads the engine's tiles on the copy stream, while the next rs_engine_upload_async, rs_engine_infer and
 * the staging copy of rs_engine_infer_device / _phase write them on the engine's stream.  An event recorded behind the kernel orders
 * those writes behind it while a band-histogram fetch is outstanding; an engine that never uses the add-on enqueues what it always
 * did.  rs_engine_fetch_band_hist_wait waits for the copy (and for whatever else is on the copy stream in front of it). */
typedef struct rs_band_hist {
  uint32_t* hist;       /* [tile_first[n]][C][256], capacity max_batch * RS_EVAL_GT_CAP * C * 256 */
} rs_band_hist;
int rs_engine_fetch_band_hist_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                    const int32_t* inst_first, const int32_t* tile_first, rs_band_hist* out);
int rs_engine_fetch_band_hist_wait(rs_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* RS_ENGINE_H */
