// librs_engine.so host side: the training engine, the rs_trainer_* entries of include/rs_engine.h.  It drives
// the stages, activations and weight blob of its forward engine directly (engine_internal.h).
//
// What detectron2's SimpleTrainer.run_step does with autograd ([EXT d2: engine/train_loop.py; modeling/meta_arch/rcnn.py
// GeneralizedRCNN.forward]) is laid out here as an explicit backward stage list over the forward engine's buffers:
//   * the forward engine keeps every layer output in its own buffer, so nothing is recomputed or stashed;
//   * every gradient w.r.t. an activation has a buffer of the same NHWC-with-halo geometry ("d:<tensor>");
//   * input gradients run through the forward implicit-GEMM kernel on a transposed, tap-flipped fp16 copy of the
//     weight, with the ReLU mask / identity add / fp32 RoIAlign scatter / 2x2 down-sum fused into its epilogue;
//   * weight gradients run through conv_wgrad.hip into one flat fp32 gradient buffer laid out like the flat fp32
//     master-weight buffer (forward GEMM layout, UNFOLDED: the trainable tensor is the raw convolution weight, the
//     FrozenBN scale is applied by the fold and by the weight-gradient reduce);
//   * one SGD-momentum launch updates the whole flat buffer, one fold launch per layer regenerates the two fp16 operands.
// Stage A (this file, round 1): trunk backward (FPN + res5..res3) from given gradients of p2..p6, checked against the
// training oracle's autograd.  The loss/label kernels (train_kernels.hip) and the RoI-head backward are wired in next.
#include <string.h>

#include <cmath>

#include "engine_internal.h"
#include "polygon_pool.h"
#include "train.h"
#include "train_stats.h"

namespace {

struct TrainLayer {
  std::string name;              // engine layer name, e.g. "backbone.bottom_up.res3.0.conv1"
  int Cout = 0, Cin = 0, KH = 1, KW = 1, Kpad = 0, KpadT = 0;
  size_t w_off = 0;              // offset (floats) of the weight in master / grad / momentum
  size_t b_off = (size_t)-1;     // offset of the trainable bias, (size_t)-1 = none (FrozenBN bias is constant)
  half_t* w_fwd = nullptr;       // engine's fp16 forward weight (rewritten by the fold every step)
  float* b_fwd = nullptr;        // engine's fp32 bias
  half_t* w_bwd = nullptr;       // [Cin][KpadT] transposed, tap-flipped fp16 copy for the input gradient (null = not needed)
  const float* scale = nullptr;  // FrozenBN scale [Cout] (null = none)
  half_t* w_bwd_planes = nullptr; // split input-gradient mode: [2 * Cin][KpadT] hi / lo fp16 planes of the row-scaled w_bwd (allocated at switch-on)
  float* w_bwd_inv = nullptr;     //   and the inverse row scales [Cin]
  bool x_stage = false;           // an add_dgrad stage reads w_bwd (the mask deconvolution's direct call does not go through it)
  int bias_tile = 1;             // forward bias = master bias repeated this many times (the 2x2 deconv as 4 GEMMs)
};

}  // namespace

struct rs_trainer {
  rs_engine* eng = nullptr;
  bool f32 = false;              // reference-precision trainer (rs_spec.precision = 1): activations, gradients and GEMM operands are fp32
  int freeze_at = 2;             // MODEL.BACKBONE.FREEZE_AT (rs_train_options): 2 = stem and res2 frozen, 1 = res2 trained, 0 = the stem too
  int first_stage() const { return freeze_at < 2 ? 0 : 1; }   // first trainable residual stage (index into rs_spec.res_blocks)
  size_t esz() const { return f32 ? 4 : 2; }
  int edt() const { return f32 ? DT_F32 : DT_F16; }
  int N = 0;
  hipStream_t stream = nullptr;
  std::vector<TrainLayer> layers;
  std::map<std::string, int> lidx;
  float *master = nullptr, *grad = nullptr, *mom = nullptr;
  size_t n_params = 0;
  float* partial = nullptr;
  // weight / bias gradients leave the input-gradient chain: they only READ finished buffers (dy of their layer, the forward
  // activation) and write the flat gradient + the `partial` scratch, which nothing on the main stream touches during a
  // backward list -- so they run on a side stream next to the chain's (often latency-bound) kernels.
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int run_list(std::vector<Stage>& list, int n);
  int join_side();
  bool side_pending = false;
  // RoIAlign backward (L2-atomic-bound, ~2 ms of a batch-8 step) also runs on the side stream; the chain waits for it right
  // before the first consumer of the fp32 maps (the RPN conv's input gradient of p2), not at the end of its list
  bool roi_bwd_on_side = true;
  hipEvent_t ev_dp32 = nullptr;
  bool dp32_pending = false;
  // RPN targets (anchor Matcher + subsample) computed ahead of the step on the side stream (rs_trainer_rpn_targets_async): they depend on the
  // ground truth and the seed only, not on anything the network computes
  hipEvent_t ev_rpn_targets = nullptr;
  bool rpn_targets_ready = false;
  uint32_t rpn_targets_seed = 0;
  FoldDesc* fold_table = nullptr;   // every layer's fold (and bias copies) as one launch; built on the first fold_all()
  int fold_n = 0;
  unsigned fold_blocks = 0;
  size_t partial_floats = 0;
  half_t* zeros = nullptr;       // zero fp16 row (wgrad tail rows)
  // weight gradients on split operands (rs_trainer_set_wgrad_mode; fp32 trainer only): hi + lo fp16 planes of the dY and X of the stage
  // that is running -- the `*.w` stages follow one another on one stream, so one scratch serves them all
  int wgrad_mode = 0;
  void* wgs_scratch = nullptr;
  long long wgs_dy_cap = 0, wgs_x_cap = 0;   // elements of the largest dY / X of any weight-gradient stage
  void wgs_note(long long dy_el, long long x_el) { if (dy_el > wgs_dy_cap) wgs_dy_cap = dy_el; if (x_el > wgs_x_cap) wgs_x_cap = x_el; }
  void wgs_apply(WgradParams& p) const {
    p.split_ops = f32 && wgrad_mode == 1;
    p.split_scratch = wgs_scratch; p.split_dy_cap = wgs_dy_cap; p.split_x_cap = wgs_x_cap;
  }
  // input gradients on split operands (rs_trainer_set_dgrad_mode; fp32 trainer only): hi + lo fp16 planes of the dY of the `*.x` stage
  // that is running.  Those stages follow one another on the chain stream, so one scratch of the chain's own serves them all (the
  // weight-gradient scratch above belongs to the side stream); the planes of every w_bwd are rewritten behind each fold.
  int dgrad_mode = 0;
  void* dgs_scratch = nullptr;
  long long dgs_cap = 0;           // elements of the largest dY of any add_dgrad stage
  SplitRowsDesc* dgs_table = nullptr;
  int dgs_n = 0;
  unsigned dgs_rows = 0;
  int split_w_bwd();               // w_bwd of every layer -> planes + inverse row scales, one launch on the chain stream
  // forward product on split operands (rs_trainer_set_fwd_mode; fp32 trainer only): the mode, its X scratch and the weight planes live in
  // the forward engine (rs_engine::fwd_mode), whose conv / linear stages read it when they launch; fold_all() re-splits behind the fold
  std::set<const void*> folded_weights() const;
  float* zero_bias = nullptr;    // zero fp32 bias for input-gradient convolutions
  std::vector<void*> allocs;
  std::vector<TensorInfo> tensors;
  std::map<std::string, Act> dact;
  std::vector<Stage> bwd;        // trunk backward stages, in execution order
  std::vector<Stage> rpn_bwd;    // RPN targets, losses and head backward (runs before the trunk backward)
  std::vector<Stage>* cur = nullptr;   // list add_dgrad / add_wgrad append to
  // ---- targets and RPN training state
  static constexpr int GT_CAP = 128;
  float* gt_boxes = nullptr;     // [N][GT_CAP][4] network-input pixels
  int* gt_classes = nullptr;     // [N][GT_CAP]
  int* gt_count = nullptr;       // [N]
  float* anchors = nullptr;      // [A_total][4], (level, y, x, a) order
  int A_total = 0, level_off[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int* rpn_matched = nullptr;    // [N][A_total]
  int* rpn_labels = nullptr;     // [N][A_total] 1 / 0 / -1 (after subsampling)
  unsigned int* gt_best = nullptr;
  float* losses = nullptr;       // [8]: rpn_cls, rpn_loc, cls, box_reg, mask
  LossScratch loss_scratch[3] = {};   // rpn / box / mask loss: the logged sums in a fixed order (train.h), so that two runs of a step log the same bits
  int rpn_first_stage = -1, rpn_last_stage = -1;
  unsigned int seed = 1;
  bool external_rpn_labels = false;   // parity tests: keep the labels the caller wrote into rpn_labels
  int rpn_batch = 256, roi_batch = 1024;                 // R:223, R:178
  float rpn_pos_frac = 0.5f, roi_pos_frac = 0.25f;       // R:246, R:192
  // ---- RoI box head training state
  std::vector<Stage> roi_bwd;    // box loss + box head backward + RoIAlign backward (runs before rpn_bwd)
  static constexpr int CAND_CAP = 1024 + GT_CAP, PC = 1024;
  float* dP32[4] = {nullptr, nullptr, nullptr, nullptr};   // fp32 gradient maps of p2..p5 (RoIAlign-backward scatter target)
  size_t dP32_bytes[4] = {0, 0, 0, 0};
  RoiSampleParams rsp;
  // training-mode proposal generation: PRE_NMS_TOPK_TRAIN 2000 per level, POST_NMS_TOPK_TRAIN 1000 per image (R:248,250)
  RpnParams t_rp;
  NmsParams t_nms;
  RpnMergeParams t_merge;
  int rpn_pre_topk_train = 2000, rpn_post_topk_train = 1000;
  int* roi_sampled = nullptr;    // [N][PC]
  int* roi_sampled_count = nullptr;
  int prop_first_stage = -1, box_first_stage = -1, box_last_stage = -1;
  bool roi_grads_valid = false;
  bool rpn_forward_done = false;  // set by rs_trainer_rpn_forward, cleared by rs_trainer_forward_trunk: rpn_step then skips the head forward
  // ---- mask head training state
  std::vector<Stage> mask_fwd, mask_bwd;
  static constexpr int MEI = 256;      // mask-head entries per image: BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION (R:178,192)
  int* m_slots = nullptr;
  int* m_cls = nullptr;
  int* m_total = nullptr;
  uint8_t* m_targets = nullptr;   // [N*MEI][28*28]
  uint8_t* m_targets_pinned = nullptr;   // host staging of the targets (pinned: the upload needs no stream sync)
  hipEvent_t ev_targets = nullptr;       // the staging buffer's last upload
  hipStream_t copy = nullptr;            // read-back of the sampled RoIs while the box head runs
  hipEvent_t ev_rois = nullptr;          // sampled RoIs written (recorded inside rs_trainer_roi_step)
  float* h_boxes = nullptr; int32_t* h_gti = nullptr; int32_t* h_cnt = nullptr;   // pinned read-back buffers
  // ---- mask targets rasterised on the device (opt-in: rs_trainer_set_polygons + rs_trainer_mask_backward_device).  The polygon pool
  // holds the ground-truth polygons of ONE batch: at most N * MT_POLYS_PER_IMAGE polygons and N * MT_DOUBLES_PER_IMAGE doubles
  // (N = the trainer's batch capacity; 32 768 vertices and 512 KiB per image on average); a batch beyond that is the caller's to
  // rasterise on the host (RS_POLYGONS_DO_NOT_FIT).  Pool and staging are allocated by the first rs_trainer_set_polygons.
  static constexpr int MT_POLYS_PER_IMAGE = 512, MT_DOUBLES_PER_IMAGE = 65536;
  uint8_t* mt_pool = nullptr;            // device, MtLayout of the current batch
  uint8_t* mt_pinned = nullptr;          // host staging of the pool
  hipEvent_t ev_polys = nullptr;         // the staging buffer's last upload
  MtLayout mt_layout;
  bool mt_set = false;                   // polygons of the current targets are in the pool (cleared by rs_trainer_set_targets)
  int mt_n = 0;
  Stage mt_stage;                        // "mask.targets": listed by rs_trainer_stage_info once the pool exists
  bool mt_listed = false;
  std::vector<TensorInfo> named;         // readable through rs_trainer_tensor by name, not part of the enumerated table
  // ---- training diagnostics (opt-in: rs_trainer_set_train_stats; train_stats.h).  Three counting stages behind the loss stages add
  // into one int32 table, zeroed where `losses` is; table and stages exist from the first switch-on, outside the lists as mt_stage is
  int train_stats_on = 0;
  int* train_stats = nullptr;            // [TS_TABLE]
  Stage ts_box, ts_mask, ts_rpn;         // "box.stats", "mask.stats", "rpn.stats": listed by rs_trainer_stage_info once switched on
  bool ts_listed = false;
  int run_stats(Stage& st, int n) { return train_stats_on ? run_stage(st, n, stream) : (int)RS_OK; }
  // ---- solver (opt-in: rs_trainer_set_solver; sgd_rule.h).  The segment table lists the trainable tensors in buffer order; the chunk
  // table, the norm scratch and the tensors "grad_norms" / "clip_coef" exist from the first set_solver.  Never set: apply_sgd is the
  // two launches it always was.
  struct Segment { std::string name; size_t off = 0, count = 0; int bias = 0; };
  std::vector<Segment> segments;
  const std::vector<Segment>& segment_table() {
    if (segments.empty())
      for (const TrainLayer& L : layers) {
        Segment w;
        w.name = L.name + ".w"; w.off = L.w_off; w.count = (size_t)L.Cout * L.Kpad; w.bias = 0;
        segments.push_back(w);
        if (L.b_off != (size_t)-1) {
          Segment b;
          b.name = L.name + ".b"; b.off = L.b_off; b.count = (size_t)L.Cout; b.bias = 1;
          segments.push_back(b);
        }
      }
    return segments;
  }
  bool solver_on = false;
  rs_solver solver = {};
  SgdPlan sgd_plan = {};
  const int* ctx_m_count = nullptr;   // while set, add_dgrad / add_wgrad bound their rows by this device counter (entries)
  int build_mask_training();
  std::vector<std::pair<void*, size_t>> clear_list;   // gradient buffers that must be zero before a backward pass
  int trunk_last_stage = -1;     // index of the engine's last trunk stage (fpn.p6)
  float loss_scale = 1.f;
  int* overflow = nullptr;       // [1] set by rs_trainer_apply_sgd when the gradient held inf / nan (the step was skipped)
  float grad_divisor = 1.f;      // extra division of the gradients in the SGD step (world size after an all-reduce SUM)
  long long step_count = 0;
  // ---- gradient buckets (data-parallel all-reduce overlapped with the backward pass).  The flat gradient buffer is laid out
  // [res3 | res4 | res5 | fpn | heads] (add_layer order; with FREEZE_AT below 2 [res2 | in front of it, at 0 [stem | in front of that);
  // a step finishes the groups in the order heads (box, mask, RPN: complete after rs_trainer_rpn_step), fpn, res5, res4, res3
  // (trunk backward), then res2 and stem where they are trained.  Each bucket is one contiguous range with two
  // events (chain stream / weight-gradient side stream) recorded right after its last writer has been enqueued, so a collective
  // on another stream can start behind them while the rest of the backward is still running (rs_trainer_bucket_wait).
  struct GradBucket {
    std::string name;
    size_t off = 0, count = 0;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    int last_trunk_stage = -1;   // index in `bwd` of the last stage that writes this bucket (-1: not written by the trunk list)
  };
  std::vector<GradBucket> buckets;     // readiness order
  hipEvent_t ev_foreign = nullptr;
  int bucket_of(const std::string& layer) const {
    const char* pre[] = {"backbone.bottom_up.res5", "backbone.bottom_up.res4", "backbone.bottom_up.res3", "backbone.bottom_up.res2",
                         "backbone.bottom_up.stem"};
    if (layer.rfind("backbone.fpn", 0) == 0) return 1;
    for (int i = 0; i < 5; ++i) if (layer.rfind(pre[i], 0) == 0) return 2 + i;
    return 0;
  }
  int build_buckets();
  int record_bucket(int b);
  // ---- per-stage HIP-event timing of a step (bench.py --train): events around every stage on the stream it runs on, no host wait;
  // resolved by rs_trainer_stage_count / _stage_info
  int profiling = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pev;
  std::vector<Stage*> pev_stage;
  std::vector<int> pev_n;
  size_t pev_used = 0;
  std::vector<Stage*> all_stages;    // engine forward stages of the training step, then roi_bwd, mask_fwd, mask_bwd, rpn_bwd, bwd
  int run_stage(Stage& st, int n, hipStream_t s);
  int resolve_profile();

  int alloc(void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    RS_HIP(hipMalloc(p, bytes));
    allocs.push_back(*p);
    RS_HIP(hipMemsetAsync(*p, 0, bytes, stream));
    return RS_OK;
  }
  void reg(const std::string& name, void* p, int dtype, std::vector<int64_t> dims, int halo) {
    TensorInfo t;
    t.name = name; t.p = p; t.dtype = dtype; t.ndim = (int)dims.size(); t.halo = halo;
    size_t nb = dt_size(dtype);
    for (size_t i = 0; i < dims.size(); ++i) { t.dims[i] = dims[i]; nb *= (size_t)dims[i]; }
    t.bytes = nb;
    tensors.push_back(t);
  }
  // forward activation of the engine by tensor name
  int fwd_act(const std::string& name, Act* a) {
    for (const TensorInfo& t : eng->tensors)
      if (t.name == name) {
        RS_CHECK(t.dtype == edt() && t.ndim == 4, RS_ERR_ARG, "tensor %s is not an activation of the trainer's precision", name.c_str());
        a->p = (half_t*)t.p; a->N = (int)t.dims[0]; a->pad = t.halo;
        a->H = (int)t.dims[1] - 2 * t.halo; a->W = (int)t.dims[2] - 2 * t.halo; a->C = (int)t.dims[3];
        return RS_OK;
      }
    rs_set_error("trainer: forward tensor %s not found", name.c_str());
    return RS_ERR_ARG;
  }
  // gradient buffer with the geometry of forward tensor `name` (created on first use)
  int grad_act(const std::string& name, Act* a, bool needs_clear = false) {
    auto it = dact.find(name);
    if (it != dact.end()) { *a = it->second; return RS_OK; }
    Act f;
    int rc = fwd_act(name, &f);
    if (rc) return rc;
    *a = f;
    const size_t bytes = (size_t)f.N * f.Hp() * f.Wp() * f.C * esz();
    rc = alloc((void**)&a->p, bytes);
    if (rc) return rc;
    reg("d:" + name, a->p, edt(), {f.N, f.Hp(), f.Wp(), f.C}, f.pad);
    dact[name] = *a;
    if (needs_clear) clear_list.emplace_back((void*)a->p, bytes);
    return RS_OK;
  }
  int add_layer(const std::string& name, int KH, int KW, bool needs_dgrad, bool has_bias);
  int add_dgrad(const std::string& stage, const std::string& layer, const Act& dy, const Act& dx, int stride, int pad, const Act* res,
                const Act* mask, const Act* down, const float* res32 = nullptr, int rows_per_image = 0);
  int add_wgrad(const std::string& stage, const std::string& layer, const Act& dy, const Act& x, int stride, int pad, bool accumulate = false,
                int rows_per_image = 0);
  int build_box_training();
  int build_trunk_backward();
  int build_rpn_training();
  int fold_all();
};

int rs_trainer::add_layer(const std::string& name, int KH, int KW, bool needs_dgrad, bool has_bias) {
  const BlobEntry* m = eng->find(name + ".m32");
  const BlobEntry* w = eng->find(name + (f32 ? ".w32" : ".w"));
  const BlobEntry* b = eng->find(name + ".b");
  RS_CHECK(m && w && b, RS_ERR_BLOB, "trainer: layer %s lacks .m32/.w/.b in the blob (pack with train=True)", name.c_str());
  RS_CHECK(m->dtype == DT_F32 && m->dims[0] == w->dims[0] && m->dims[1] == w->dims[1], RS_ERR_BLOB, "trainer: %s master/forward shapes differ", name.c_str());
  TrainLayer L;
  L.name = name;
  L.Cout = (int)w->dims[0]; L.Kpad = (int)w->dims[1]; L.KH = KH; L.KW = KW;
  RS_CHECK(L.Kpad % (KH * KW) == 0, RS_ERR_BLOB, "trainer: %s K %d not divisible by %dx%d taps", name.c_str(), L.Kpad, KH, KW);
  L.Cin = L.Kpad / (KH * KW);
  L.w_fwd = (half_t*)w->dev; L.b_fwd = (float*)b->dev;
  const BlobEntry* s = eng->find(name + ".s");
  L.scale = s ? (const float*)s->dev : nullptr;
  L.w_off = n_params;
  n_params += (size_t)L.Cout * L.Kpad;
  if (has_bias) { L.b_off = n_params; n_params += (size_t)((L.Cout + 63) / 64 * 64); }
  if (needs_dgrad) {
    const int kc = (L.Cout + 63) / 64 * 64;            // K of the input-gradient GEMM: (taps, Cout padded to 64)
    L.KpadT = KH * KW * kc;
    int rc = alloc((void**)&L.w_bwd, (size_t)L.Cin * L.KpadT * esz());
    if (rc) return rc;
  }
  // scratch for the split partial tiles: wgrad_splits() never exceeds ceil(1024 / output tiles) (and 64)
  // (reference precision: wgrad_splits aims at 1280 workgroups of 64 channels x 4 K-column tiles)
  const long long out_tiles = f32 ? (long long)cdiv(L.Cout, 64) * cdiv(KH * KW * (L.Cin >> 6), 4) : (long long)cdiv(L.Cout, 128) * cdiv(KH * KW * (L.Cin >> 6), 2);
  long long smax = cdiv(f32 ? 1280 : 1024, out_tiles);
  if (smax > 64) smax = 64;
  const size_t pf = (size_t)smax * L.Cout * L.Kpad;
  if (pf > partial_floats) partial_floats = pf;
  lidx[name] = (int)layers.size();
  layers.push_back(L);
  return RS_OK;
}

// dx = mask * (conv_transpose(dy) + res + 2x2-sum(down)); stride > 1 (1x1 only): scattered store into the caller-zeroed dx
int rs_trainer::add_dgrad(const std::string& stage, const std::string& layer, const Act& dy, const Act& dx, int stride, int pad,
                          const Act* res, const Act* mask, const Act* down, const float* res32, int rows_per_image) {
  auto it = lidx.find(layer);
  RS_CHECK(it != lidx.end() && layers[it->second].w_bwd, RS_ERR_ARG, "trainer: no input-gradient weights for %s", layer.c_str());
  const TrainLayer& L = layers[it->second];
  RS_CHECK(stride == 1 || (L.KH == 1 && L.KW == 1), RS_ERR_UNSUPPORTED, "trainer: %s stride %d with a %dx%d kernel", layer.c_str(), stride, L.KH, L.KW);
  const int pad_t = L.KH - 1 - pad;
  RS_CHECK(dy.pad >= pad_t && dy.C % 64 == 0 && dy.C * L.KH * L.KW == L.KpadT, RS_ERR_ARG, "trainer: %s gradient geometry (C %d, KpadT %d)", layer.c_str(), dy.C, L.KpadT);
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.in = dy.p; p.w = L.w_bwd; p.bias = zero_bias; p.out = dx.p;
  p.res = res ? res->p : nullptr;
  p.res32 = res32;
  p.mask = mask ? mask->p : nullptr;
  p.Ho = stride == 1 ? dx.H : dy.H; p.Wo = stride == 1 ? dx.W : dy.W;
  p.in_Hp = dy.Hp(); p.in_Wp = dy.Wp(); p.in_Cs = dy.C; p.in_off = dy.pad - pad_t;
  p.stride = 1; p.KH = L.KH; p.KW = L.KW; p.Cin = dy.C; p.Kpad = L.KpadT; p.Cout = dx.C;
  p.out_Hp = dx.Hp(); p.out_Wp = dx.Wp(); p.out_Cs = dx.C; p.out_pad = dx.pad;
  p.out_stride = stride;
  if (down) { p.down = down->p; p.down_Hp = down->Hp(); p.down_Wp = down->Wp(); p.down_Cs = down->C; p.down_pad = down->pad; }
  RS_CHECK(dx.C == L.Cin, RS_ERR_ARG, "trainer: %s dx channels %d != Cin %d", layer.c_str(), dx.C, L.Cin);
  if (res) RS_CHECK(res->H == dx.H && res->W == dx.W && res->C == dx.C && res->pad == dx.pad, RS_ERR_ARG, "trainer: %s residual geometry", stage.c_str());
  if (mask) RS_CHECK(mask->H == dx.H && mask->W == dx.W && mask->C == dx.C && mask->pad == dx.pad, RS_ERR_ARG, "trainer: %s mask geometry", stage.c_str());
  const int mpi = rows_per_image > 0 ? rows_per_image : p.Ho * p.Wo;
  if (ctx_m_count) { p.m_count = ctx_m_count; p.m_mul = p.Ho * p.Wo; }
  Stage st;
  st.name = stage;
  st.flops_per_image = 2.0 * mpi * (double)L.KH * L.KW * L.Cout * L.Cin;
  const int glds = f32 ? -1 : 1;
  const long long dy_el = (long long)dy.N * dy.Hp() * dy.Wp() * dy.C;
  if (dy_el > dgs_cap) dgs_cap = dy_el;
  // the mode is read when the stage launches: split operands where the kernel serves the shape, else (and in mode 0) the fp32 kernel
  const bool served = f32 && conv_dgrad_split_serves(dx.C, dy.C, L.KH, L.KW, stride);
  rs_trainer* self = this;
  const int li = it->second;
  layers[li].x_stage = true;
  st.fn = [p, mpi, glds, served, self, li](int n, hipStream_t s) mutable {
    p.M = n * mpi;
    if (!(served && self->dgrad_mode == 1)) return launch_conv(p, s, -1, glds);
    const TrainLayer& TL = self->layers[li];
    ConvParams q = p;                          // q.in: the fp32 dY
    int rc = launch_dgrad_split_planes(q, self->dgs_scratch, self->dgs_cap, s);
    if (rc) return rc;
    q.split = 1; q.dy_amax = (const unsigned*)self->dgs_scratch;
    q.in = (const half_t*)((const char*)self->dgs_scratch + WGS_HEAD_BYTES); q.in_lo = self->dgs_cap;
    q.w = TL.w_bwd_planes; q.w_lo = (long long)TL.Cin * TL.KpadT; q.wscale = TL.w_bwd_inv;
    return launch_conv(q, s, -1, 1);
  };
  (cur ? cur : &bwd)->push_back(st);
  return RS_OK;
}

int rs_trainer::add_wgrad(const std::string& stage, const std::string& layer, const Act& dy, const Act& x, int stride, int pad, bool accumulate,
                          int rows_per_image) {
  auto it = lidx.find(layer);
  RS_CHECK(it != lidx.end(), RS_ERR_ARG, "trainer: unknown layer %s", layer.c_str());
  const TrainLayer& L = layers[it->second];
  RS_CHECK(x.pad >= pad && x.C == L.Cin && dy.C >= L.Cout, RS_ERR_ARG, "trainer: %s weight-gradient geometry", layer.c_str());
  WgradParams p;
  memset(&p, 0, sizeof p);
  p.dy = dy.p; p.x = x.p; p.scale = L.scale; p.zeros = zeros;
  p.Ho = dy.H; p.Wo = dy.W;
  p.dy_Hp = dy.Hp(); p.dy_Wp = dy.Wp(); p.dy_Cs = dy.C; p.dy_pad = dy.pad;
  p.in_Hp = x.Hp(); p.in_Wp = x.Wp(); p.in_Cs = x.C; p.in_off = x.pad - pad;
  p.stride = stride; p.KH = L.KH; p.KW = L.KW; p.Cin = L.Cin; p.Cout = L.Cout; p.Kpad = L.Kpad;
  if (ctx_m_count) { p.m_count = ctx_m_count; p.m_mul = dy.H * dy.W; }
  p.f32 = f32 ? 1 : 0;
  const int* mc = ctx_m_count;
  const int mc_mul_bias = dy.Hp() * dy.Wp();
  const size_t w_off = L.w_off;
  const int mpi = rows_per_image > 0 ? rows_per_image : dy.H * dy.W;
  rs_trainer* self = this;
  Stage st;
  st.name = stage;
  st.flops_per_image = 2.0 * mpi * (double)L.KH * L.KW * L.Cout * L.Cin;
  st.fn = [p, mpi, self, w_off, accumulate](int n, hipStream_t s) mutable {
    p.M = n * mpi;
    p.partial = self->partial;
    p.grad = self->grad + w_off;
    p.accumulate = accumulate ? 1 : 0;
    self->wgs_apply(p);
    p.splits = wgrad_splits(p);
    return launch_conv_wgrad(p, s);
  };
  wgs_note((long long)dy.N * dy.Hp() * dy.Wp() * dy.C, (long long)x.N * x.Hp() * x.Wp() * x.C);
  st.grad_side = true;
  st.bucket = bucket_of(layer);
  (cur ? cur : &bwd)->push_back(st);
  if (L.b_off != (size_t)-1) {
    const size_t b_off = L.b_off;
    const half_t* dyp = dy.p;
    const int C = dy.C, cout = L.Cout;
    const long long rpi = rows_per_image > 0 ? rows_per_image : (long long)dy.Hp() * dy.Wp();
    Stage sb;
    sb.name = stage + ".bias";
    sb.fn = [dyp, rpi, C, cout, self, b_off, accumulate, mc, mc_mul_bias](int n, hipStream_t s) {
      return launch_bias_grad(dyp, (long long)n * rpi, C, cout, self->grad + b_off, accumulate ? 1 : 0, s, mc, mc_mul_bias, self->partial, self->f32 ? 1 : 0);   // halo rows are zero
    };
    sb.grad_side = true;
    sb.bucket = st.bucket;
    (cur ? cur : &bwd)->push_back(sb);
  }
  return RS_OK;
}

int rs_trainer::run_stage(Stage& st, int n, hipStream_t s) {
  const bool rec = profiling && pev_used < pev.size();
  if (rec) RS_HIP(hipEventRecord(pev[pev_used].first, s));
  int rc = st.fn(n, s);
  if (rc) { rs_set_error("%s (stage %s)", rs_last_error(), st.name.c_str()); return rc; }
  if (rec) {
    RS_HIP(hipEventRecord(pev[pev_used].second, s));
    pev_stage[pev_used] = &st;
    pev_n[pev_used] = n;
    ++pev_used;
  }
  return RS_OK;
}

int rs_trainer::resolve_profile() {
  if (pev_used == 0) return RS_OK;
  RS_HIP(hipStreamSynchronize(stream));
  if (side) RS_HIP(hipStreamSynchronize(side));
  for (size_t i = 0; i < pev_used; ++i) {
    float ms = 0.f;
    RS_HIP(hipEventElapsedTime(&ms, pev[i].first, pev[i].second));
    Stage& st = *pev_stage[i];
    st.ms_total += ms;
    st.calls += 1;
    st.last_flops = st.flops_per_image * pev_n[i];
  }
  pev_used = 0;
  return RS_OK;
}

int rs_trainer::run_list(std::vector<Stage>& list, int n) {
  bool forked = false;
  for (Stage& st : list) {
    hipStream_t s = stream;
    if (st.grad_side && side) {
      RS_HIP(hipEventRecord(ev_fork, stream));          // everything the chain has produced so far, including this layer's dy
      RS_HIP(hipStreamWaitEvent(side, ev_fork, 0));
      s = side;
      forked = true;
    }
    int rc = run_stage(st, n, s);
    if (rc) return rc;
    if (s == side && side && st.name.size() >= 9 && st.name.compare(st.name.size() - 9, 9, "roi_align") == 0) {
      RS_HIP(hipEventRecord(ev_dp32, side));            // the fp32 RoIAlign-gradient maps are complete up to here
      dp32_pending = true;
    }
    if (&list == &bwd && st.bucket >= 0) {
      const int idx = (int)(&st - &list[0]);
      if (st.bucket < (int)buckets.size() && buckets[st.bucket].last_trunk_stage == idx) {
        rc = record_bucket(st.bucket);
        if (rc) return rc;
      }
    }
  }
  // No join here: the side stream only writes the flat gradient and its scratch, and reads buffers the chain does not touch
  // again before the next forward -- the chain waits for it where that matters (join_side: next forward, SGD step, sync).
  if (forked) side_pending = true;
  return RS_OK;
}

int rs_trainer::join_side() {
  if (!side_pending) return RS_OK;
  RS_HIP(hipEventRecord(ev_join, side));
  RS_HIP(hipStreamWaitEvent(stream, ev_join, 0));
  side_pending = false;
  dp32_pending = false;
  return RS_OK;
}

// every writer of bucket b has been enqueued: mark the point on both streams
int rs_trainer::record_bucket(int b) {
  if (b < 0 || b >= (int)buckets.size()) return RS_OK;
  RS_HIP(hipEventRecord(buckets[b].ev_main, stream));
  if (side) RS_HIP(hipEventRecord(buckets[b].ev_side, side));
  return RS_OK;
}

int rs_trainer::build_buckets() {
  static const char* names[] = {"heads", "fpn", "res5", "res4", "res3", "res2", "stem"};
  const int nb = 5 + (2 - freeze_at);          // FREEZE_AT 1 adds res2, 0 also stem: they finish after res3, in this order
  buckets.assign(nb, GradBucket());
  std::vector<size_t> lo(nb, (size_t)-1), hi(nb, 0);
  for (size_t i = 0; i < layers.size(); ++i) {
    const TrainLayer& L = layers[i];
    const int b = bucket_of(L.name);
    const size_t end = i + 1 < layers.size() ? layers[i + 1].w_off : n_params;   // the layer's weight, bias and padding
    if (L.w_off < lo[b]) lo[b] = L.w_off;
    if (end > hi[b]) hi[b] = end;
  }
  size_t covered = 0;
  for (int b = 0; b < nb; ++b) {
    RS_CHECK(lo[b] != (size_t)-1, RS_ERR_ARG, "trainer: gradient bucket %s is empty", names[b]);
    buckets[b].name = names[b]; buckets[b].off = lo[b]; buckets[b].count = hi[b] - lo[b];
    covered += buckets[b].count;
    RS_HIP(hipEventCreateWithFlags(&buckets[b].ev_main, hipEventDisableTiming));
    RS_HIP(hipEventCreateWithFlags(&buckets[b].ev_side, hipEventDisableTiming));
  }
  // contiguous, disjoint, complete: a layer of one group between two layers of another would make the ranges overlap
  RS_CHECK(covered == n_params, RS_ERR_ARG, "trainer: gradient buckets cover %zu of %zu values (layer order changed?)", covered, n_params);
  for (size_t i = 0; i < bwd.size(); ++i)
    if (bwd[i].bucket > 0) buckets[bwd[i].bucket].last_trunk_stage = (int)i;
  RS_HIP(hipEventCreateWithFlags(&ev_foreign, hipEventDisableTiming));
  return RS_OK;
}

// master -> fp16 operands of every layer (forward weight with the FrozenBN scale folded, input-gradient copy) + biases
int rs_trainer::fold_all() {
  if (!fold_table) {
    std::vector<FoldDesc> tab;
    unsigned blocks = 0;
    auto push = [&](FoldDesc d) { d.block_start = blocks; blocks += fold_desc_blocks(d); tab.push_back(d); };
    for (const TrainLayer& L : layers) {
      FoldDesc d = {};
      d.w32 = master + L.w_off; d.scale = L.scale; d.fwd = L.w_fwd; d.bwd = L.w_bwd;
      d.Cout = L.Cout; d.Cin = L.Cin; d.KH = L.KH; d.KW = L.KW; d.Kpad = L.Kpad; d.kc = (L.Cout + 63) / 64 * 64; d.KpadT = L.KpadT;
      d.f32 = f32 ? 1 : 0;
      RS_CHECK(d.w32 && d.fwd && (!d.bwd || d.KH * d.KW * d.kc <= d.KpadT), RS_ERR_ARG, "fold: bad layer %s", L.name.c_str());
      push(d);
      if (L.b_off != (size_t)-1) {
        FoldDesc b = {};
        b.w32 = master + L.b_off; b.fwd32 = L.b_fwd; b.Cin = L.Cout; b.KH = L.bias_tile;
        push(b);
      }
      if (L.name == "roi_heads.mask_head.predictor16") {
        // the INFERENCE mask head reads the predictor as fp32 [K][256] (VALU dot on the predicted class, fused into the deconv): keep
        // it in step so that the trainer's engine can run validation inference (rs_trainer_engine) with the current weights
        const BlobEntry* pw = eng->find("roi_heads.mask_head.predictor.w");
        const BlobEntry* pb = eng->find("roi_heads.mask_head.predictor.b");
        if (pw && pb) {
          FoldDesc c = {};
          c.w32 = master + L.w_off; c.fwd32 = (float*)pw->dev; c.Cin = (int)(pw->dims[0] * pw->dims[1]); c.KH = 1;
          push(c);
          c.w32 = master + L.b_off; c.fwd32 = (float*)pb->dev; c.Cin = (int)pb->dims[0];
          push(c);
        }
      }
    }
    int rc = alloc((void**)&fold_table, tab.size() * sizeof(FoldDesc));
    if (rc) return rc;
    RS_HIP(hipMemcpyAsync(fold_table, tab.data(), tab.size() * sizeof(FoldDesc), hipMemcpyHostToDevice, stream));
    RS_HIP(hipStreamSynchronize(stream));      // tab is a local
    fold_n = (int)tab.size(); fold_blocks = blocks;
  }
  int rc = launch_fold_table(fold_table, fold_n, fold_blocks, stream);
  if (!rc && dgrad_mode == 1) rc = split_w_bwd();
  if (!rc && eng->fwd_mode == 1) rc = eng->fwd_split_weights(/*folded_only=*/true);      // the split forward's planes of what the fold rewrote
  return rc;
}

// the forward weights a fold rewrites (everything else the forward engine reads is frozen: the stem and res2 at FREEZE_AT 2, the stem at 1)
std::set<const void*> rs_trainer::folded_weights() const {
  std::set<const void*> s;
  for (const TrainLayer& L : layers) s.insert((const void*)L.w_fwd);
  return s;
}

int rs_trainer::split_w_bwd() {
  RS_CHECK(dgs_table && dgs_n > 0, RS_ERR_ARG, "trainer: the split input-gradient mode has no weight planes");
  return launch_split_rows_table(dgs_table, dgs_n, dgs_rows, stream);
}

// FPN and res5..res3 backward from d:p2..d:p6 (FREEZE_AT 2: nothing flows into res2 / the stem); FREEZE_AT 1 goes on through res2
// (weight gradients only in res2.0, whose input is the frozen stem output), FREEZE_AT 0 through res2.0 into d:stem, the max-pool and
// the stem's weight gradient (stem_bwd.hip).  The stem has no input gradient.
int rs_trainer::build_trunk_backward() {
  const rs_spec& S = eng->spec;
  int rc;
  const std::string bu = "backbone.bottom_up.";
  const int first = first_stage();
  const bool stem_trained = freeze_at == 0;
  // ---- layers (execution order of the forward): [stem, res2,] res3..res5, FPN
  if (stem_trained) {
    // the stem's [64][RS_STEM_KPAD] GEMM operand as a 1x1 layer over its 256 K columns: the fold scales its rows, nothing transposes it
    RS_CHECK(S.stem_out_channels == 64, RS_ERR_UNSUPPORTED, "trainer: MODEL.BACKBONE.FREEZE_AT 0 needs a 64-channel stem, this one has %d", S.stem_out_channels);
    if ((rc = add_layer(bu + "stem.conv1", 1, 1, false, false))) return rc;
    const TrainLayer& L = layers.back();
    RS_CHECK(L.Cout == 64 && L.Kpad == RS_STEM_KPAD, RS_ERR_BLOB, "trainer: stem weight is %d x %d, expected 64 x %d", L.Cout, L.Kpad, RS_STEM_KPAD);
    const size_t pf = (size_t)RS_STEM_WGRAD_MAX_SPLITS * 64 * RS_STEM_KPAD;
    if (pf > partial_floats) partial_floats = pf;
  }
  for (int si = first; si < 4; ++si) {
    // block 0 of a stage needs its two input-gradient operands when something trainable lies below it
    const bool below = si > first || (si == 0 && stem_trained);
    for (int bi = 0; bi < S.res_blocks[si]; ++bi) {
      const std::string wn = bu + "res" + std::to_string(si + 2) + "." + std::to_string(bi);
      if (bi == 0) { if ((rc = add_layer(wn + ".shortcut", 1, 1, below, false))) return rc; }
      if ((rc = add_layer(wn + ".conv1", 1, 1, bi > 0 || below, false))) return rc;   // FREEZE_AT 2: res3.0 reads the frozen res2
      if ((rc = add_layer(wn + ".conv2", 3, 3, true, false))) return rc;
      if ((rc = add_layer(wn + ".conv3", 1, 1, true, false))) return rc;
    }
  }
  for (int l = 2; l <= 5; ++l) {
    if ((rc = add_layer("backbone.fpn_lateral" + std::to_string(l), 1, 1, l - 2 >= first, true))) return rc;
    if ((rc = add_layer("backbone.fpn_output" + std::to_string(l), 3, 3, true, true))) return rc;
  }

  // ---- gradient buffers of the FPN outputs (filled by the heads' backward / the test hook)
  Act dP[5], P[5];
  for (int l = 0; l < 5; ++l) {
    const std::string nm = "p" + std::to_string(l + 2);
    if ((rc = fwd_act(nm, &P[l]))) return rc;
    if ((rc = grad_act(nm, &dP[l]))) return rc;
  }
  // p6 = max_pool2d(p5, k=1, s=2): its gradient lands on the even pixels of d:p5
  {
    const Act a = dP[4], b = dP[3];
    Stage st;
    st.name = "bwd.fpn.p6";
    const int f = f32 ? 1 : 0;
    st.fn = [a, b, f](int n, hipStream_t s) { return launch_subsample2_bwd(a.p, b.p, n, b.H, b.W, a.H, a.W, 256, s, f); };
    bwd.push_back(st);
  }
  // ---- FPN: finest level first (inner_l feeds inner_{l-1} through the nearest upsample)
  Act dInner[4], inner[4], res[4];
  for (int l = 0; l < 4; ++l) {
    const std::string ln = std::to_string(l + 2);
    if ((rc = fwd_act("inner" + ln, &inner[l]))) return rc;
    if ((rc = fwd_act("res" + ln, &res[l]))) return rc;
    if ((rc = grad_act("inner" + ln, &dInner[l]))) return rc;
    if ((rc = add_wgrad("bwd.fpn_output" + ln + ".w", "backbone.fpn_output" + ln, dP[l], inner[l], 1, 1))) return rc;
    if ((rc = add_dgrad("bwd.fpn_output" + ln + ".x", "backbone.fpn_output" + ln, dP[l], dInner[l], 1, 1, nullptr, nullptr,
                        l > 0 ? &dInner[l - 1] : nullptr))) return rc;
    if ((rc = add_wgrad("bwd.fpn_lateral" + ln + ".w", "backbone.fpn_lateral" + ln, dInner[l], res[l], 1, 0))) return rc;
  }
  // ---- res5 .. res3 (.. res2)
  for (int si = 3; si >= first; --si) {
    const std::string sn = "res" + std::to_string(si + 2);
    const int nb = S.res_blocks[si];
    // gradient w.r.t. the stage output: lateral input gradient + what the next stage's first block scattered, ReLU-masked
    Act dOut;
    if ((rc = grad_act(sn, &dOut, si < 3))) return rc;
    if ((rc = add_dgrad("bwd.fpn_lateral" + std::to_string(si + 2) + ".x", "backbone.fpn_lateral" + std::to_string(si + 2), dInner[si], dOut, 1, 0,
                        si < 3 ? &dOut : nullptr, &res[si], nullptr))) return rc;
    Act G = dOut;                                   // d(pre-ReLU block output), masked
    for (int bi = nb - 1; bi >= 0; --bi) {
      const std::string nm = sn + "." + std::to_string(bi);
      const std::string wn = bu + nm;
      const int stride = (bi == 0 && si > 0) ? 2 : 1;      // res2.0 is a projection block at the stem output's resolution
      Act t1, t2, x, dT1, dT2;
      if ((rc = fwd_act(nm + ".conv1", &t1))) return rc;
      if ((rc = fwd_act(nm + ".conv2", &t2))) return rc;
      const std::string xin = bi == 0 ? (si == 0 ? std::string("stem") : "res" + std::to_string(si + 1))
                                      : (bi - 1 == nb - 1 ? sn : sn + "." + std::to_string(bi - 1) + ".out");
      if ((rc = fwd_act(xin, &x))) return rc;
      if ((rc = grad_act(nm + ".conv1", &dT1))) return rc;
      if ((rc = grad_act(nm + ".conv2", &dT2))) return rc;
      if ((rc = add_wgrad("bwd." + nm + ".conv3.w", wn + ".conv3", G, t2, 1, 0))) return rc;
      if ((rc = add_dgrad("bwd." + nm + ".conv3.x", wn + ".conv3", G, dT2, 1, 0, nullptr, &t2, nullptr))) return rc;
      if ((rc = add_wgrad("bwd." + nm + ".conv2.w", wn + ".conv2", dT2, t1, 1, 1))) return rc;
      if ((rc = add_dgrad("bwd." + nm + ".conv2.x", wn + ".conv2", dT2, dT1, 1, 1, nullptr, &t1, nullptr))) return rc;
      if ((rc = add_wgrad("bwd." + nm + ".conv1.w", wn + ".conv1", dT1, x, S.stride_in_1x1 ? stride : 1, 0))) return rc;
      RS_CHECK(S.stride_in_1x1 || stride == 1, RS_ERR_UNSUPPORTED, "trainer: STRIDE_IN_1X1 false is not supported");
      if (bi > 0) {
        // identity shortcut: d(x) = relu'(x) * (conv1 input gradient + G)
        Act dX;
        if ((rc = grad_act(xin, &dX))) return rc;
        if ((rc = add_dgrad("bwd." + nm + ".conv1.x", wn + ".conv1", dT1, dX, 1, 0, &G, &x, nullptr))) return rc;
        G = dX;
      } else {
        if ((rc = add_wgrad("bwd." + nm + ".shortcut.w", wn + ".shortcut", G, x, stride, 0))) return rc;
        if (si > first) {
          // projection block: both 1x1 stride-2 input gradients land on the even pixels of d(res_{si-1}) (zeroed before the
          // pass); the lateral input gradient of that stage adds them up and applies the ReLU mask
          Act dX;
          if ((rc = grad_act(xin, &dX, true))) return rc;
          if ((rc = add_dgrad("bwd." + nm + ".conv1.x", wn + ".conv1", dT1, dX, stride, 0, nullptr, nullptr, nullptr))) return rc;
          if ((rc = add_dgrad("bwd." + nm + ".shortcut.x", wn + ".shortcut", G, dX, stride, 0, &dX, nullptr, nullptr))) return rc;
        } else if (si == 0 && stem_trained) {
          // res2.0 at stride 1: the two input gradients cover every pixel of d:stem, the second adds the first.  The stem output is a
          // max-pool's, so there is no mask here: the ReLU mask is applied on stem_conv by the pool's backward.
          Act dX;
          if ((rc = grad_act(xin, &dX))) return rc;
          if ((rc = add_dgrad("bwd." + nm + ".conv1.x", wn + ".conv1", dT1, dX, 1, 0, nullptr, nullptr, nullptr))) return rc;
          if ((rc = add_dgrad("bwd." + nm + ".shortcut.x", wn + ".shortcut", G, dX, 1, 0, &dX, nullptr, nullptr))) return rc;
        }
      }
    }
  }
  if (stem_trained) {
    // ---- stem: d:stem -> max-pool + ReLU backward -> d:stem_conv -> weight gradient against the network input
    Act sc, x0, dS, dSC;
    if ((rc = fwd_act("stem_conv", &sc))) return rc;
    if ((rc = fwd_act("net_input", &x0))) return rc;
    if ((rc = grad_act("stem", &dS))) return rc;
    if ((rc = grad_act("stem_conv", &dSC))) return rc;
    RS_CHECK(sc.C == 64 && x0.C == 4 && x0.pad >= 3 && x0.H == 2 * sc.H && x0.W == 2 * sc.W && dS.C == sc.C, RS_ERR_ARG, "trainer: stem geometry");
    PoolBwdParams pp;
    memset(&pp, 0, sizeof pp);
    pp.x = sc.p; pp.dq = dS.p; pp.dx = dSC.p;
    pp.Hc = sc.H; pp.Wc = sc.W; pp.Hq = dS.H; pp.Wq = dS.W; pp.C = sc.C; pp.x_halo = sc.pad; pp.q_halo = dS.pad;
    pp.f32 = f32 ? 1 : 0;
    Stage sp;
    sp.name = "bwd.stem.maxpool";
    sp.fn = [pp](int n, hipStream_t s) mutable { pp.N = n; return launch_maxpool3x3s2_bwd(pp, s); };
    bwd.push_back(sp);
    const std::string layer = bu + "stem.conv1";
    const TrainLayer& L = layers[lidx[layer]];
    StemWgradParams wp;
    memset(&wp, 0, sizeof wp);
    wp.dy = dSC.p; wp.x0 = x0.p; wp.scale = L.scale;
    wp.Hc = sc.H; wp.Wc = sc.W; wp.dy_halo = dSC.pad; wp.x_halo = x0.pad; wp.cin = S.in_channels;
    wp.f32 = f32 ? 1 : 0;
    rs_trainer* self = this;
    const size_t w_off = L.w_off;
    Stage sw;
    sw.name = "bwd.stem.conv1.w";
    sw.flops_per_image = 2.0 * sc.H * sc.W * 49.0 * S.in_channels * 64;
    sw.fn = [wp, self, w_off](int n, hipStream_t s) mutable {
      wp.N = n;
      wp.partial = self->partial;
      wp.grad = self->grad + w_off;
      wp.splits = stem_wgrad_splits((long long)n * wp.Hc * wp.Wc);
      return launch_stem_wgrad(wp, s);
    };
    sw.grad_side = true;
    sw.bucket = bucket_of(layer);
    bwd.push_back(sw);
  }
  return RS_OK;
}

// RPN training: anchors, Matcher (0.3 / 0.7, low-quality matches), subsample (256 @ 0.5), losses per level, and the
// backward of the shared head (1x1 heads + 3x3 conv, gradients accumulated over the five levels) into d:p2..d:p6
// ([EXT d2: modeling/proposal_generator/rpn.py RPN.forward(training) / label_and_sample_anchors / losses]).
int rs_trainer::build_rpn_training() {
  const rs_spec& S = eng->spec;
  const int A = S.num_anchors, L = S.num_levels;
  const int head_cs = (5 * A + 15) / 16 * 16;
  int rc;
  for (size_t i = 0; i < eng->stages.size(); ++i) {
    const std::string& nm = eng->stages[i].name;
    if (nm.rfind("rpn.conv", 0) == 0 || nm.rfind("rpn.heads", 0) == 0) {
      if (rpn_first_stage < 0) rpn_first_stage = (int)i;
      rpn_last_stage = (int)i;
    }
  }
  // 2 L stages (3x3 and heads per level), or L + 1 when the shared 3x3 of all levels is one multi-map launch ("rpn.conv2-6")
  RS_CHECK(rpn_first_stage == trunk_last_stage + 1 && (rpn_last_stage == rpn_first_stage + 2 * L - 1 || rpn_last_stage == rpn_first_stage + L), RS_ERR_ARG, "trainer: unexpected RPN stage layout");
  cur = &rpn_bwd;
  if ((rc = add_layer("proposal_generator.rpn_head.conv", 3, 3, true, true))) return rc;
  if ((rc = add_layer("proposal_generator.rpn_head.heads", 1, 1, true, true))) return rc;
  // ---- anchors (DefaultAnchorGenerator: shifts arange(offset*stride, size*stride, stride), order (y, x, a))
  Act P[8], T[8];
  std::vector<float> host;
  for (int l = 0; l < L; ++l) {
    if ((rc = fwd_act("p" + std::to_string(l + 2), &P[l]))) return rc;
    if ((rc = fwd_act("rpn_conv" + std::to_string(l + 2), &T[l]))) return rc;
    level_off[l] = A_total;
    const float stride = (float)(4 << l);
    for (int y = 0; y < P[l].H; ++y)
      for (int x = 0; x < P[l].W; ++x)
        for (int a = 0; a < A; ++a) {
          const float sx = S.anchor_offset * stride + (float)x * stride, sy = S.anchor_offset * stride + (float)y * stride;
          host.push_back(sx + S.cell_anchors[l][a][0]); host.push_back(sy + S.cell_anchors[l][a][1]);
          host.push_back(sx + S.cell_anchors[l][a][2]); host.push_back(sy + S.cell_anchors[l][a][3]);
        }
    A_total += P[l].H * P[l].W * A;
  }
  if ((rc = alloc((void**)&anchors, host.size() * 4))) return rc;
  RS_HIP(hipMemcpyAsync(anchors, host.data(), host.size() * 4, hipMemcpyHostToDevice, stream));
  RS_HIP(hipStreamSynchronize(stream));
  reg("anchors", anchors, DT_F32, {A_total, 4}, 0);
  if ((rc = alloc((void**)&gt_boxes, (size_t)N * GT_CAP * 16))) return rc;
  if ((rc = alloc((void**)&gt_classes, (size_t)N * GT_CAP * 4))) return rc;
  if ((rc = alloc((void**)&gt_count, (size_t)N * 4))) return rc;
  if ((rc = alloc((void**)&rpn_matched, (size_t)N * A_total * 4))) return rc;
  if ((rc = alloc((void**)&rpn_labels, (size_t)N * A_total * 4))) return rc;
  if ((rc = alloc((void**)&gt_best, (size_t)N * GT_CAP * 4))) return rc;
  if ((rc = alloc((void**)&losses, 8 * 4))) return rc;
  if ((rc = alloc((void**)&overflow, 4))) return rc;
  reg("grad_overflow", overflow, DT_I32, {1}, 0);
  reg("rpn_labels", rpn_labels, DT_I32, {N, A_total}, 0);
  reg("rpn_matched", rpn_matched, DT_I32, {N, A_total}, 0);
  reg("losses", losses, DT_F32, {8}, 0);
  reg("gt_boxes", gt_boxes, DT_F32, {N, GT_CAP, 4}, 0);
  for (int l = 0; l < 4 && l < L; ++l) {
    dP32_bytes[l] = (size_t)N * P[l].Hp() * P[l].Wp() * 256 * 4;
    if ((rc = alloc((void**)&dP32[l], dP32_bytes[l]))) return rc;
    reg("d32:p" + std::to_string(l + 2), dP32[l], DT_F32, {N, P[l].Hp(), P[l].Wp(), 256}, P[l].pad);
  }
  rs_trainer* self = this;
  // ---- targets
  {
    Stage st;
    st.name = "rpn.match";
    st.fn = [self](int n, hipStream_t s) {
      if (self->external_rpn_labels) return RS_OK;
      if (self->rpn_targets_ready && self->rpn_targets_seed == self->seed) {      // computed ahead on the side stream: the chain only waits for them
        RS_HIP(hipStreamWaitEvent(s, self->ev_rpn_targets, 0));
        return (int)RS_OK;
      }
      self->rpn_targets_ready = false;
      MatchParams m;
      memset(&m, 0, sizeof m);
      m.boxes = self->anchors; m.gt = self->gt_boxes; m.gt_count = self->gt_count; m.matched = self->rpn_matched; m.labels = self->rpn_labels;
      m.gt_best = self->gt_best; m.n_boxes = self->A_total; m.gt_cap = GT_CAP;
      m.t_lo = 0.3f; m.t_hi = 0.7f; m.lbl_lo = 0; m.lbl_mid = -1; m.lbl_hi = 1;          // R:237-243
      return launch_match(m, n, s);
    };
    rpn_bwd.push_back(st);
    Stage sb;
    sb.name = "rpn.subsample";
    sb.fn = [self](int n, hipStream_t s) {
      if (self->external_rpn_labels) return RS_OK;
      if (self->rpn_targets_ready && self->rpn_targets_seed == self->seed) { self->rpn_targets_ready = false; return (int)RS_OK; }
      SubsampleParams q;
      memset(&q, 0, sizeof q);
      q.labels = self->rpn_labels; q.n = self->A_total; q.num_samples = self->rpn_batch; q.positive_fraction = self->rpn_pos_frac; q.bg_label = 0; q.rpn_mode = 1;
      q.seed = self->seed * 2654435761u + 17u;
      return launch_subsample(q, n, s);
    };
    rpn_bwd.push_back(sb);
  }
  // ---- per level: loss -> heads backward -> conv backward
  for (int l = 0; l < L; ++l) {
    const std::string ln = std::to_string(l + 2);
    float* head = nullptr;
    for (const TensorInfo& t : eng->tensors) if (t.name == "rpn_head" + ln) head = (float*)t.p;
    RS_CHECK(head, RS_ERR_ARG, "trainer: rpn_head%s missing", ln.c_str());
    Act dH;                                    // gradient of the fused head output, 64 channels wide (one K step of the input-gradient GEMM)
    dH.N = N; dH.H = P[l].H; dH.W = P[l].W; dH.C = 64; dH.pad = 0;
    if ((rc = alloc((void**)&dH.p, (size_t)N * dH.H * dH.W * 64 * esz()))) return rc;
    reg("d:rpn_head" + ln, dH.p, edt(), {N, dH.H, dH.W, 64}, 0);
    const int hw = P[l].H * P[l].W, loff = level_off[l];
    Stage st;
    st.name = "rpn.loss" + ln;
    st.fn = [self, head, dH, hw, loff, A, head_cs](int n, hipStream_t s) {
      RpnLossParams q;
      memset(&q, 0, sizeof q);
      q.head = head; q.dhead = dH.p; q.labels = self->rpn_labels; q.anchors = self->anchors; q.gt = self->gt_boxes; q.matched = self->rpn_matched;
      q.loss_out = self->losses; q.A = A; q.cs = head_cs; q.dcs = 64; q.HW = hw; q.n_anchors = hw * A; q.level_off = loff;
      q.total_anchors = self->A_total; q.gt_cap = GT_CAP; q.normalizer = (float)self->rpn_batch * (float)n; q.loss_scale = self->loss_scale;
      q.d32 = self->f32 ? 1 : 0;
      q.scratch = self->loss_scratch[0];
      return launch_rpn_loss(q, n, s);
    };
    rpn_bwd.push_back(st);
    Act dT, dP;
    if ((rc = grad_act("rpn_conv" + ln, &dT))) return rc;
    if ((rc = grad_act("p" + ln, &dP))) return rc;
    if ((rc = add_wgrad("bwd.rpn.heads" + ln + ".w", "proposal_generator.rpn_head.heads", dH, T[l], 1, 0, l > 0))) return rc;
    if ((rc = add_dgrad("bwd.rpn.heads" + ln + ".x", "proposal_generator.rpn_head.heads", dH, dT, 1, 0, nullptr, &T[l], nullptr))) return rc;
    if ((rc = add_wgrad("bwd.rpn.conv" + ln + ".w", "proposal_generator.rpn_head.conv", dT, P[l], 1, 1, l > 0))) return rc;
    if (l == 0) {
      Stage sw;
      sw.name = "rpn.wait_roi_align_bwd";
      sw.fn = [self](int, hipStream_t s) {
        if (self->dp32_pending) { RS_HIP(hipStreamWaitEvent(s, self->ev_dp32, 0)); self->dp32_pending = false; }
        return (int)RS_OK;
      };
      rpn_bwd.push_back(sw);
    }
    // d:p_l = input gradient of the RPN conv + what RoIAlign-backward scattered into the fp32 map (p2..p5)
    if ((rc = add_dgrad("bwd.rpn.conv" + ln + ".x", "proposal_generator.rpn_head.conv", dT, dP, 1, 1, nullptr, nullptr, nullptr, l < 4 ? dP32[l] : nullptr))) return rc;
  }
  cur = nullptr;
  return RS_OK;
}

// RoI box head training ([EXT d2: modeling/roi_heads/roi_heads.py StandardROIHeads.forward(training)]): RPN proposals (+ gt),
// Matcher at 0.5, subsample (1024 @ 0.25), then the ENGINE's box-head forward stages run on the sampled boxes (they are
// written into its fixed 1024-slot proposal buffer), FastRCNNOutputLayers.losses, and the backward of predictor / fc2 /
// fc1 / RoIAlign into the fp32 maps d32:p2..p5.
int rs_trainer::build_box_training() {
  const rs_spec& S = eng->spec;
  int rc;
  for (size_t i = 0; i < eng->stages.size(); ++i) {
    const std::string& nm = eng->stages[i].name;
    if (nm == "rpn.select_decode") prop_first_stage = (int)i;
    if (nm == "box.roi_align") box_first_stage = (int)i;
    if (nm == "box.predictor") box_last_stage = (int)i;
  }
  RS_CHECK(prop_first_stage == rpn_last_stage + 1 && box_first_stage == prop_first_stage + 3 && box_last_stage == box_first_stage + 3, RS_ERR_ARG,
           "trainer: unexpected proposal / box-head stage layout");
  cur = &roi_bwd;
  if ((rc = add_layer("roi_heads.box_head.fc1", 1, 1, true, true))) return rc;
  if ((rc = add_layer("roi_heads.box_head.fc2", 1, 1, true, true))) return rc;
  if ((rc = add_layer("roi_heads.box_predictor", 1, 1, true, true))) return rc;
  const int K = S.num_classes, PR = S.box_pooler_resolution;
  const int pred_cs = (5 * K + 1 + 15) / 16 * 16;
  auto dev_tensor = [&](const char* name) -> void* { for (const TensorInfo& t : eng->tensors) if (t.name == name) return t.p; return nullptr; };
  float* prop_boxes = (float*)dev_tensor("proposal_boxes");
  int* prop_count = (int*)dev_tensor("proposal_count");
  float* pred = (float*)dev_tensor("box_pred");
  half_t* pooled = (half_t*)dev_tensor("box_pooled");
  RS_CHECK(prop_boxes && prop_count && pred && pooled, RS_ERR_ARG, "trainer: box-head tensors missing");
  {
    // the engine's own proposal stages are sized for inference (1000 per level); training keeps 2000 per level before NMS
    const int L = S.num_levels, A = S.num_anchors, CAPT = 2048;
    memset(&t_rp, 0, sizeof t_rp);
    for (int l = 0; l < L; ++l) {
      Act P;
      if ((rc = fwd_act("p" + std::to_string(l + 2), &P))) return rc;
      t_rp.head[l] = (const float*)dev_tensor(("rpn_head" + std::to_string(l + 2)).c_str());
      RS_CHECK(t_rp.head[l], RS_ERR_ARG, "trainer: rpn_head%d missing", l + 2);
      t_rp.H[l] = P.H; t_rp.W[l] = P.W; t_rp.stride[l] = 4 << l;
      if ((rc = alloc((void**)&t_rp.keys[l], (size_t)N * P.H * P.W * A * 4 * 2))) return rc;
      for (int a = 0; a < A; ++a)
        for (int d = 0; d < 4; ++d) t_rp.base[l][a][d] = S.cell_anchors[l][a][d];
    }
    t_rp.offset = S.anchor_offset; t_rp.L = L; t_rp.A = A; t_rp.cs = (5 * A + 15) / 16 * 16; t_rp.cand_cap = CAPT;
    t_rp.img_h = (float)eng->net_h; t_rp.img_w = (float)eng->net_w; t_rp.img_hw = eng->img_hw_dev;
    t_rp.wx = S.rpn_bbox_reg_weights[0]; t_rp.wy = S.rpn_bbox_reg_weights[1]; t_rp.ww = S.rpn_bbox_reg_weights[2]; t_rp.wh = S.rpn_bbox_reg_weights[3];
    t_rp.scale_clamp = S.scale_clamp; t_rp.min_size = S.rpn_min_size;
    uint8_t* keepb = nullptr;
    if ((rc = alloc((void**)&t_rp.cand_boxes, (size_t)N * L * CAPT * 16))) return rc;
    if ((rc = alloc((void**)&t_rp.cand_scores, (size_t)N * L * CAPT * 4))) return rc;
    if ((rc = alloc((void**)&t_rp.cand_valid, (size_t)N * L * CAPT))) return rc;
    if ((rc = alloc((void**)&t_rp.cand_count, (size_t)N * L * 4))) return rc;
    if ((rc = alloc((void**)&keepb, (size_t)N * L * CAPT))) return rc;
    t_nms = NmsParams{};
    t_nms.boxes = t_rp.cand_boxes; t_nms.count = t_rp.cand_count; t_nms.valid = t_rp.cand_valid; t_nms.keep = keepb; t_nms.cap = CAPT;
    t_nms.thresh = S.rpn_nms_thresh;
    if ((rc = alloc((void**)&t_nms.scratch, (size_t)N * L * CAPT * (CAPT / 64) * 8))) return rc;
    if (S.batched_nms) {
      // find_top_rpn_proposals calls the same batched_nms in training: at most 1000 valid candidates per image take the shifted form
      // (out of reach at PRE_NMS_TOPK_TRAIN 2000 x 5 levels on real maps; rs_trainer_set_rpn_topk and small inputs get there)
      if ((rc = alloc((void**)&t_nms.rule, (size_t)N * 2 * 4))) return rc;
      if ((rc = alloc((void**)&t_nms.unit, (size_t)N * 4))) return rc;
      reg("train_rpn_nms_rule", t_nms.rule, DT_I32, {N, 2}, 0);
      reg("train_rpn_nms_unit", t_nms.unit, DT_F32, {N}, 0);
      t_nms.group = L;
    }
    t_merge = RpnMergeParams{};
    t_merge.cand_boxes = t_rp.cand_boxes; t_merge.cand_scores = t_rp.cand_scores; t_merge.keep = keepb; t_merge.cand_count = t_rp.cand_count;
    t_merge.L = L; t_merge.cap = PC; t_merge.cand_cap = CAPT;
    t_merge.prop_boxes = prop_boxes; t_merge.prop_count = prop_count;
    t_merge.prop_scores = (float*)dev_tensor("proposal_logits");
    t_merge.prop_level = (int*)dev_tensor("proposal_level");
    RS_CHECK(t_merge.prop_scores, RS_ERR_ARG, "trainer: proposal_logits missing");
  }
  memset(&rsp, 0, sizeof rsp);
  rsp.prop_boxes = prop_boxes; rsp.prop_count = prop_count; rsp.gt_boxes = gt_boxes; rsp.gt_classes = gt_classes; rsp.gt_count = gt_count;
  rsp.prop_cap = PC; rsp.gt_cap = GT_CAP; rsp.cand_cap = CAND_CAP; rsp.out_cap = PC; rsp.K = K;
  if ((rc = alloc((void**)&rsp.cand_boxes, (size_t)N * CAND_CAP * 16))) return rc;
  if ((rc = alloc((void**)&rsp.cand_count, (size_t)N * 4))) return rc;
  if ((rc = alloc((void**)&rsp.matched, (size_t)N * CAND_CAP * 4))) return rc;
  if ((rc = alloc((void**)&rsp.labels, (size_t)N * CAND_CAP * 4))) return rc;
  if ((rc = alloc((void**)&roi_sampled, (size_t)N * PC * 4))) return rc;
  if ((rc = alloc((void**)&roi_sampled_count, (size_t)N * 2 * 4))) return rc;
  if ((rc = alloc((void**)&rsp.out_classes, (size_t)N * PC * 4))) return rc;
  if ((rc = alloc((void**)&rsp.out_gt_boxes, (size_t)N * PC * 16))) return rc;
  if ((rc = alloc((void**)&rsp.out_gt_index, (size_t)N * PC * 4))) return rc;
  rsp.sampled = roi_sampled; rsp.sampled_count = roi_sampled_count;
  rsp.out_boxes = prop_boxes; rsp.out_count = prop_count;          // the sampled set replaces the proposals in the engine's buffer
  reg("roi_candidates", rsp.cand_boxes, DT_F32, {N, CAND_CAP, 4}, 0);
  reg("roi_candidate_count", rsp.cand_count, DT_I32, {N}, 0);
  reg("roi_classes", rsp.out_classes, DT_I32, {N, PC}, 0);
  reg("roi_gt_boxes", rsp.out_gt_boxes, DT_F32, {N, PC, 4}, 0);
  reg("roi_gt_index", rsp.out_gt_index, DT_I32, {N, PC}, 0);
  reg("roi_sampled_count", roi_sampled_count, DT_I32, {N, 2}, 0);
  reg("roi_boxes", prop_boxes, DT_F32, {N, PC, 4}, 0);
  rs_trainer* self = this;
  // ---- loss
  Act dPred;                                       // gradient of the fused predictor output, 64 channels wide
  dPred.N = 1; dPred.H = N * PC; dPred.W = 1; dPred.C = 64; dPred.pad = 0;
  if ((rc = alloc((void**)&dPred.p, (size_t)N * PC * 64 * esz()))) return rc;
  reg("d:box_pred", dPred.p, edt(), {N, PC, 64}, 0);
  {
    Stage st;
    st.name = "box.loss";
    st.fn = [self, pred, dPred, K, pred_cs](int n, hipStream_t s) {
      BoxLossParams q;
      memset(&q, 0, sizeof q);
      q.pred = pred; q.dpred = dPred.p; q.gt_classes = self->rsp.out_classes; q.proposals = self->rsp.out_boxes; q.gt_boxes = self->rsp.out_gt_boxes;
      q.loss_out = self->losses + 2; q.n_rois = n * PC; q.K = K; q.cs = pred_cs; q.dcs = 64;
      q.n_valid_counts = self->roi_sampled_count; q.n_valid_n = n;
      q.wx = self->eng->spec.box_reg_weights[0]; q.wy = self->eng->spec.box_reg_weights[1];
      q.ww = self->eng->spec.box_reg_weights[2]; q.wh = self->eng->spec.box_reg_weights[3];
      q.loss_scale = self->loss_scale;
      q.d32 = self->f32 ? 1 : 0;
      q.scratch = self->loss_scratch[1];
      return launch_box_loss(q, s);
    };
    roi_bwd.push_back(st);
  }
  // ---- backward: predictor, fc2, fc1 (linear layers = 1x1 convolutions over an (M x 1) image), RoIAlign
  Act f1, f2, fin, dF1, dF2, dPool;
  if ((rc = fwd_act("box_fc1", &f1))) return rc;
  if ((rc = fwd_act("box_fc2", &f2))) return rc;
  fin.p = pooled; fin.N = 1; fin.H = N * PC; fin.W = 1; fin.C = PR * PR * 256; fin.pad = 0;
  if ((rc = grad_act("box_fc1", &dF1))) return rc;
  if ((rc = grad_act("box_fc2", &dF2))) return rc;
  dPool = fin;
  if ((rc = alloc((void**)&dPool.p, (size_t)N * PC * PR * PR * 256 * esz()))) return rc;
  reg("d:box_pooled", dPool.p, edt(), {N * PC, PR, PR, 256}, 0);
  if ((rc = add_wgrad("bwd.box.predictor.w", "roi_heads.box_predictor", dPred, f2, 1, 0, false, PC))) return rc;
  if ((rc = add_dgrad("bwd.box.predictor.x", "roi_heads.box_predictor", dPred, dF2, 1, 0, nullptr, &f2, nullptr, nullptr, PC))) return rc;
  if ((rc = add_wgrad("bwd.box.fc2.w", "roi_heads.box_head.fc2", dF2, f1, 1, 0, false, PC))) return rc;
  if ((rc = add_dgrad("bwd.box.fc2.x", "roi_heads.box_head.fc2", dF2, dF1, 1, 0, nullptr, &f1, nullptr, nullptr, PC))) return rc;
  if ((rc = add_wgrad("bwd.box.fc1.w", "roi_heads.box_head.fc1", dF1, fin, 1, 0, false, PC))) return rc;
  if ((rc = add_dgrad("bwd.box.fc1.x", "roi_heads.box_head.fc1", dF1, dPool, 1, 0, nullptr, nullptr, nullptr, nullptr, PC))) return rc;
  {
    RoiAlignParams q;
    memset(&q, 0, sizeof q);
    for (int l = 0; l < 4; ++l) {
      Act P;
      if ((rc = fwd_act("p" + std::to_string(l + 2), &P))) return rc;
      q.dfeat[l] = dP32[l]; q.H[l] = P.H; q.W[l] = P.W; q.scale[l] = 1.0f / (float)(4 << l);
    }
    q.nlevels = 4; q.C = 256; q.rois = prop_boxes; q.per_image_count = prop_count; q.slots_per_image = PC; q.out = dPool.p; q.P = PR; q.out_pad = 0;
    q.f32 = f32 ? 1 : 0;
    // owner-computes backward (roi_align.hip roi_bwd_gather_kernel): per-entry tables + the counter of entries left to the atomic kernel
    if ((rc = alloc(&q.bwd_tables, (size_t)N * PC * RS_ROI_BWD_TABLE_BYTES))) return rc;
    if ((rc = alloc((void**)&q.bwd_overflow, 64))) return rc;
    Stage st;
    st.name = "bwd.box.roi_align";
    st.fn = [q](int n, hipStream_t s) mutable { q.S = n * PC; q.n_images = n; return launch_roi_align_bwd(q, s); };
    st.grad_side = roi_bwd_on_side;       // off the chain: its fp32 maps are only read again by the RPN conv's input gradient
    roi_bwd.push_back(st);
  }
  cur = nullptr;
  return RS_OK;
}

// Mask head training ([EXT d2: modeling/roi_heads/mask_head.py BaseMaskRCNNHead.forward(training), mask_rcnn_loss]): the sampled
// FOREGROUND RoIs (select_foreground_proposals) go through RoIAlign 14x14, four 3x3 convs, the 2x2 deconv and the 1x1 predictor
// (here a 16-row GEMM with fp32 logits for every class); BCE against host-rasterised gt masks; backward of all of it into the
// fp32 maps d32:p2..p5.  Every GEMM is bounded by the device-side entry count.
int rs_trainer::build_mask_training() {
  const rs_spec& S = eng->spec;
  if (!S.mask_on) return RS_OK;
  int rc;
  const int ME = N * MEI, MR = S.mask_pooler_resolution, SD = 2 * MR;
  cur = &mask_bwd;
  for (int i = 1; i <= S.mask_num_conv; ++i)
    if ((rc = add_layer("roi_heads.mask_head.mask_fcn" + std::to_string(i), 3, 3, true, true))) return rc;
  if ((rc = add_layer("roi_heads.mask_head.predictor16", 1, 1, true, true))) return rc;
  // the deconv: trainable tensor in the [Cin][(dy,dx,co)] orientation (see weights.train_tensors)
  {
    const BlobEntry* mT = eng->find("roi_heads.mask_head.deconv.m32T");
    const BlobEntry* w = eng->find(f32 ? "roi_heads.mask_head.deconv.w32" : "roi_heads.mask_head.deconv.w");
    const BlobEntry* b = eng->find("roi_heads.mask_head.deconv.b");
    RS_CHECK(mT && w && b && mT->dims[0] == 256 && mT->dims[1] == 1024 && w->dims[0] == 1024, RS_ERR_BLOB, "trainer: deconv tensors missing (pack with train=True)");
    TrainLayer L;
    L.name = "roi_heads.mask_head.deconv";
    L.Cout = 256; L.Cin = 1024; L.KH = L.KW = 1; L.Kpad = 1024; L.KpadT = 256; L.bias_tile = 4;
    L.w_bwd = (half_t*)w->dev;                       // the fold's TRANSPOSED copy is the engine's forward weight [(dy,dx,co)][ci]
    L.b_fwd = (float*)b->dev;
    if ((rc = alloc((void**)&L.w_fwd, (size_t)256 * 1024 * esz()))) return rc;    // straight copy = input-gradient operand [ci][(dy,dx,co)]
    L.w_off = n_params; n_params += (size_t)256 * 1024;
    L.b_off = n_params; n_params += 256;
    const size_t pf = (size_t)64 * 256 * 1024;          // wgrad_splits() <= 64
    if (pf > partial_floats) partial_floats = pf;
    lidx[L.name] = (int)layers.size();
    layers.push_back(L);
  }
  if ((rc = alloc((void**)&m_slots, (size_t)ME * 4))) return rc;
  if ((rc = alloc((void**)&m_cls, (size_t)ME * 4))) return rc;
  if ((rc = alloc((void**)&m_total, 16))) return rc;
  if ((rc = alloc((void**)&m_targets, (size_t)ME * SD * SD))) return rc;
  RS_HIP(hipHostMalloc((void**)&m_targets_pinned, (size_t)ME * SD * SD, hipHostMallocDefault));
  RS_HIP(hipHostMalloc((void**)&h_boxes, (size_t)N * PC * 16, hipHostMallocDefault));
  RS_HIP(hipHostMalloc((void**)&h_gti, (size_t)N * PC * 4, hipHostMallocDefault));
  RS_HIP(hipHostMalloc((void**)&h_cnt, (size_t)N * 2 * 4, hipHostMallocDefault));
  reg("mask_slots", m_slots, DT_I32, {ME}, 0);
  reg("mask_classes", m_cls, DT_I32, {ME}, 0);
  reg("mask_total", m_total, DT_I32, {1}, 0);
  {
    TensorInfo ti;
    ti.name = "mask_targets"; ti.p = m_targets; ti.dtype = DT_U8; ti.ndim = 3; ti.halo = 0;
    ti.dims[0] = ME; ti.dims[1] = SD; ti.dims[2] = SD;
    ti.bytes = (size_t)ME * SD * SD;
    named.push_back(ti);
  }
  {
    rs_trainer* me = this;
    mt_stage.name = "mask.targets";
    mt_stage.fn = [me, SD](int n, hipStream_t s) {
      const MtLayout& L = me->mt_layout;
      MaskTargetsParams q;
      memset(&q, 0, sizeof q);
      q.boxes = me->rsp.out_boxes; q.gt_index = me->rsp.out_gt_index; q.slots = me->m_slots; q.total = me->m_total;
      q.image_first = (const int*)me->mt_pool; q.inst_first = (const int*)(me->mt_pool + L.o_inst);
      q.poly_off = (const int*)(me->mt_pool + L.o_off); q.poly_len = (const int*)(me->mt_pool + L.o_len);
      q.polys = (const double*)(me->mt_pool + L.o_xy);
      q.out = me->m_targets; q.n_entries = n * MEI; q.n_inst = L.n_inst; q.slots_per_image = PC; q.S = SD;
      return launch_mask_targets(q, s);
    };
  }
  // ---- forward buffers
  auto mk = [&](Act* a, const std::string& name, int H, int W, int C, int pad) -> int {
    a->N = ME; a->H = H; a->W = W; a->C = C; a->pad = pad;
    int r = alloc((void**)&a->p, (size_t)ME * a->Hp() * a->Wp() * C * esz());
    if (!r) reg(name, a->p, edt(), {ME, a->Hp(), a->Wp(), C}, pad);
    return r;
  };
  Act mp, f[4], dec, dMp, dF[4], dDec, dLog;
  if ((rc = mk(&mp, "t:mask_pooled", MR, MR, 256, 1))) return rc;
  if ((rc = mk(&dMp, "d:t:mask_pooled", MR, MR, 256, 1))) return rc;
  for (int i = 0; i < S.mask_num_conv; ++i) {
    if ((rc = mk(&f[i], "t:mask_fcn" + std::to_string(i + 1), MR, MR, 256, 1))) return rc;
    if ((rc = mk(&dF[i], "d:t:mask_fcn" + std::to_string(i + 1), MR, MR, 256, 1))) return rc;
  }
  if ((rc = mk(&dec, "t:mask_deconv", SD, SD, 256, 0))) return rc;
  if ((rc = mk(&dDec, "d:t:mask_deconv", SD, SD, 256, 0))) return rc;
  if ((rc = mk(&dLog, "d:t:mask_logits", SD, SD, 64, 0))) return rc;
  float* logits = nullptr;
  if ((rc = alloc((void**)&logits, (size_t)ME * SD * SD * 16 * 4))) return rc;
  reg("t:mask_logits", logits, DT_F32, {ME, SD * SD, 16}, 0);
  float* prop_boxes = nullptr;
  int* roi_cls = nullptr;
  for (const TensorInfo& t : eng->tensors) if (t.name == "proposal_boxes") prop_boxes = (float*)t.p;
  for (const TensorInfo& t : tensors) if (t.name == "roi_classes") roi_cls = (int*)t.p;
  RS_CHECK(prop_boxes && roi_cls, RS_ERR_ARG, "trainer: build the box head before the mask head");
  rs_trainer* self = this;
  const int* total = m_total;
  // ---- forward stages
  {
    MaskEntriesParams q;
    q.sampled_count = roi_sampled_count; q.roi_classes = roi_cls; q.slots = m_slots; q.classes = m_cls; q.total = m_total;
    q.N = 0; q.slots_per_image = PC; q.per_image_cap = MEI; q.cap = ME;
    Stage st;
    st.name = "mask.entries";
    st.fn = [q](int n, hipStream_t s) mutable { q.N = n; return launch_mask_entries(q, s); };
    mask_fwd.push_back(st);
  }
  {
    RoiAlignParams q;
    memset(&q, 0, sizeof q);
    for (int l = 0; l < 4; ++l) {
      Act P;
      if ((rc = fwd_act("p" + std::to_string(l + 2), &P))) return rc;
      q.feat[l] = P.p; q.dfeat[l] = dP32[l]; q.H[l] = P.H; q.W[l] = P.W; q.scale[l] = 1.0f / (float)(4 << l);
    }
    q.nlevels = 4; q.C = 256; q.rois = prop_boxes; q.slot_list = m_slots; q.n_entries = m_total; q.slots_per_image = PC; q.P = MR; q.out_pad = 1;
    q.f32 = f32 ? 1 : 0;
    RoiAlignParams qf = q, qb = q;
    qf.out = mp.p;
    qb.out = dMp.p;
    if ((rc = alloc(&qb.bwd_tables, (size_t)N * MEI * RS_ROI_BWD_TABLE_BYTES))) return rc;
    if ((rc = alloc((void**)&qb.bwd_overflow, 64))) return rc;
    Stage st;
    st.name = "mask.roi_align";
    st.fn = [qf](int n, hipStream_t s) mutable { qf.S = n * MEI; return launch_roi_align(qf, s); };
    mask_fwd.push_back(st);
    Stage sb;
    sb.name = "bwd.mask.roi_align";
    sb.fn = [qb](int n, hipStream_t s) mutable { qb.S = n * MEI; qb.n_images = n; return launch_roi_align_bwd(qb, s); };
    sb.grad_side = roi_bwd_on_side;
    // appended to mask_bwd at the very end (below)
    // forward convs
    auto fwd_conv = [&](const std::string& name, const std::string& layer, const Act& in, const Act& out, int k, int pad, bool relu, int mode,
                        float* out32, int cout32) -> int {
      const BlobEntry* w = eng->find(layer + (f32 ? ".w32" : ".w"));
      const BlobEntry* b = eng->find(layer + ".b");
      RS_CHECK(w && b, RS_ERR_BLOB, "trainer: weights for %s missing", layer.c_str());
      ConvParams p;
      memset(&p, 0, sizeof p);
      p.in = in.p; p.w = (const half_t*)w->dev; p.bias = (const float*)b->dev;
      p.Ho = mode ? in.H : out.H; p.Wo = mode ? in.W : out.W;
      p.in_Hp = in.Hp(); p.in_Wp = in.Wp(); p.in_Cs = in.C; p.in_off = in.pad - pad;
      p.stride = 1; p.KH = p.KW = k; p.Cin = in.C; p.Kpad = (int)w->dims[1];
      p.relu = relu ? 1 : 0; p.mode = mode;
      if (out32) { p.out = out32; p.Cout = cout32; p.out_Cs = cout32; p.out_f32 = 1; p.out_Hp = p.Ho; p.out_Wp = p.Wo; p.out_pad = 0; }
      else { p.out = out.p; p.Cout = out.C; p.out_Cs = out.C; p.out_Hp = out.Hp(); p.out_Wp = out.Wp(); p.out_pad = out.pad; }
      p.m_count = total; p.m_mul = p.Ho * p.Wo;
      const int mpi = MEI * p.Ho * p.Wo;
      const int variant = out32 ? 2 : -1;
      const int glds = f32 ? -1 : 1;
      Stage s2;
      s2.name = name;
      s2.fn = eng->conv_stage_fn(p, mpi, variant, glds);      // launch_conv(p, s, variant, glds), or the split forward in that mode
      mask_fwd.push_back(s2);
      return RS_OK;
    };
    Act curm = mp;
    for (int i = 0; i < S.mask_num_conv; ++i) {
      if ((rc = fwd_conv("mask.fcn" + std::to_string(i + 1), "roi_heads.mask_head.mask_fcn" + std::to_string(i + 1), curm, f[i], 3, 1, true, 0, nullptr, 0))) return rc;
      curm = f[i];
    }
    if ((rc = fwd_conv("mask.deconv", "roi_heads.mask_head.deconv", curm, dec, 1, 0, true, 1, nullptr, 0))) return rc;
    if ((rc = fwd_conv("mask.predictor", "roi_heads.mask_head.predictor16", dec, dec, 1, 0, false, 0, logits, 16))) return rc;
    // ---- loss
    {
      Stage sl;
      sl.name = "mask.loss";
      sl.fn = [self, logits, dLog, SD, ME](int n, hipStream_t s) {
        MaskLossParams q2;
        memset(&q2, 0, sizeof q2);
        q2.logits = logits; q2.dlogits = dLog.p; q2.targets = self->m_targets; q2.gt_classes = self->m_cls; q2.loss_out = self->losses + 4;
        q2.n_masks_ptr = self->m_total; q2.n_masks = n * MEI; q2.S = SD; q2.cs = 16; q2.dcs = 64; q2.loss_scale = self->loss_scale;
        q2.d32 = self->f32 ? 1 : 0;
        (void)ME;
        q2.scratch = self->loss_scratch[2];
        return launch_mask_loss(q2, s);
      };
      mask_bwd.push_back(sl);
    }
    // ---- backward
    ctx_m_count = m_total;
    const int per14 = MEI * MR * MR, per28 = MEI * SD * SD;
    if ((rc = add_wgrad("bwd.mask.predictor.w", "roi_heads.mask_head.predictor16", dLog, dec, 1, 0, false, per28))) return rc;
    if ((rc = add_dgrad("bwd.mask.predictor.x", "roi_heads.mask_head.predictor16", dLog, dDec, 1, 0, nullptr, &dec, nullptr, nullptr, per28))) return rc;
    {
      // deconv: weight gradient [ci][(dy,dx,co)] = sum X14[ci](y,x) * dY28[co](2y+dy, 2x+dx) (operands swapped: X14 plays the
      // "output gradient", dY28 the stride-2 2x2 "input"), bias gradient = column sum of dY28, input gradient = 2x2 stride-2
      // convolution of dY28 with the straight fp16 copy, masked by relu(fcn4)
      const TrainLayer& L = layers[lidx["roi_heads.mask_head.deconv"]];
      WgradParams p;
      memset(&p, 0, sizeof p);
      p.dy = curm.p; p.x = dDec.p; p.zeros = zeros;
      p.Ho = MR; p.Wo = MR; p.dy_Hp = curm.Hp(); p.dy_Wp = curm.Wp(); p.dy_Cs = 256; p.dy_pad = curm.pad;
      p.in_Hp = dDec.Hp(); p.in_Wp = dDec.Wp(); p.in_Cs = 256; p.in_off = 0;
      p.stride = 2; p.KH = p.KW = 2; p.Cin = 256; p.Cout = 256; p.Kpad = 1024;
      p.m_count = total; p.m_mul = MR * MR;
      p.f32 = f32 ? 1 : 0;
      const size_t w_off = L.w_off, b_off = L.b_off;
      Stage sw;
      sw.name = "bwd.mask.deconv.w";
      sw.fn = [p, per14, self, w_off](int n, hipStream_t s) mutable {
        p.M = n * per14; p.partial = self->partial; p.grad = self->grad + w_off; p.accumulate = 0;
        self->wgs_apply(p);
        p.splits = wgrad_splits(p);
        return launch_conv_wgrad(p, s);
      };
      wgs_note((long long)curm.N * curm.Hp() * curm.Wp() * curm.C, (long long)dDec.N * dDec.Hp() * dDec.Wp() * dDec.C);
      sw.grad_side = true;
      mask_bwd.push_back(sw);
      const half_t* ddp = dDec.p;
      Stage sb2;
      sb2.name = "bwd.mask.deconv.bias";
      sb2.fn = [ddp, per28, self, b_off, total, SD](int n, hipStream_t s) {
        return launch_bias_grad(ddp, (long long)n * per28, 256, 256, self->grad + b_off, 0, s, total, SD * SD, self->partial, self->f32 ? 1 : 0);
      };
      sb2.grad_side = true;
      mask_bwd.push_back(sb2);
      ConvParams c;
      memset(&c, 0, sizeof c);
      c.in = dDec.p; c.w = L.w_fwd; c.bias = zero_bias; c.out = dF[S.mask_num_conv - 1].p; c.mask = curm.p;
      c.Ho = MR; c.Wo = MR; c.in_Hp = dDec.Hp(); c.in_Wp = dDec.Wp(); c.in_Cs = 256; c.in_off = 0;
      c.stride = 2; c.KH = c.KW = 2; c.Cin = 256; c.Kpad = 1024; c.Cout = 256;
      c.out_Hp = curm.Hp(); c.out_Wp = curm.Wp(); c.out_Cs = 256; c.out_pad = curm.pad;
      c.m_count = total; c.m_mul = MR * MR;
      Stage sx;
      sx.name = "bwd.mask.deconv.x";
      const int glds = f32 ? -1 : 1;
      sx.fn = [c, per14, glds](int n, hipStream_t s) mutable { c.M = n * per14; return launch_conv(c, s, -1, glds); };
      mask_bwd.push_back(sx);
    }
    for (int i = S.mask_num_conv - 1; i >= 0; --i) {
      const std::string ln = "roi_heads.mask_head.mask_fcn" + std::to_string(i + 1);
      const Act& xin = i == 0 ? mp : f[i - 1];
      const Act& dxo = i == 0 ? dMp : dF[i - 1];
      if ((rc = add_wgrad("bwd.mask.fcn" + std::to_string(i + 1) + ".w", ln, dF[i], xin, 1, 1, false, per14))) return rc;
      if ((rc = add_dgrad("bwd.mask.fcn" + std::to_string(i + 1) + ".x", ln, dF[i], dxo, 1, 1, nullptr, i == 0 ? nullptr : &f[i - 1], nullptr, nullptr, per14))) return rc;
    }
    ctx_m_count = nullptr;
    mask_bwd.push_back(sb);
  }
  cur = nullptr;
  return RS_OK;
}

extern "C" {

int rs_trainer_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int batch, int tile_h, int tile_w,
                      int tile_c, float loss_scale, rs_trainer** out) {
  return rs_trainer_create2(spec, weights, nbytes, device_ordinal, batch, tile_h, tile_w, tile_c, loss_scale, nullptr, out);
}

int rs_trainer_freeze_at(rs_trainer* t) { return t ? t->freeze_at : -1; }

int rs_trainer_create2(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int batch, int tile_h, int tile_w,
                       int tile_c, float loss_scale, const rs_train_options* opts, rs_trainer** out) {
  RS_CHECK(spec && weights && out && loss_scale > 0.f, RS_ERR_ARG, "bad argument");
  RS_CHECK(!opts || opts->struct_size == (int32_t)sizeof(rs_train_options), RS_ERR_ARG, "rs_trainer_create2: rs_train_options.struct_size %d, expected %d",
           opts ? opts->struct_size : 0, (int)sizeof(rs_train_options));
  const int freeze_at = opts ? opts->freeze_at : 2;
  RS_CHECK(freeze_at >= 0 && freeze_at <= 2, RS_ERR_UNSUPPORTED, "trainer: MODEL.BACKBONE.FREEZE_AT %d (rs_train_options.freeze_at): 0, 1 and 2 are implemented", freeze_at);
  RS_CHECK(spec->precision == 0 || spec->precision == 1, RS_ERR_UNSUPPORTED, "trainer: precision %d", spec->precision);
  RS_CHECK(spec->num_classes <= RS_TRAIN_MAX_CLASSES, RS_ERR_UNSUPPORTED, "trainer: NUM_CLASSES %d > %d (more classes, up to %d, run in inference engines only)",
           spec->num_classes, RS_TRAIN_MAX_CLASSES, RS_MAX_CLASSES);
  rs_trainer* t = new rs_trainer();
  t->f32 = spec->precision == 1;
  t->N = batch;
  t->loss_scale = loss_scale;
  t->freeze_at = freeze_at;
  int rc = engine_create(spec, weights, nbytes, device_ordinal, batch, tile_h, tile_w, tile_c, nullptr, /*for_trainer=*/true, &t->eng, freeze_at);
  if (rc) { delete t; return rc; }
  t->stream = t->eng->stream;
  {
    if (rs_debug().train_roi_side >= 0) t->roi_bwd_on_side = rs_debug().train_roi_side != 0;
    if (rs_debug().train_side != 0) {
      // same (default) priority as the chain: measured at batch 8, 17.2 ms per step against 18.4 single-stream, while a
      // lower- or higher-priority side stream costs 19.3-19.6 ms
      if (hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&t->ev_dp32, hipEventDisableTiming) != hipSuccess) {
        rs_set_error("trainer: side stream"); rs_trainer_destroy(t); return RS_ERR_HIP;
      }
    }
  }
  if (hipStreamCreateWithFlags(&t->copy, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&t->ev_rois, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&t->ev_targets, hipEventDisableTiming) != hipSuccess) {
    rs_set_error("trainer: copy stream"); rs_trainer_destroy(t); return RS_ERR_HIP;
  }
  for (size_t i = 0; i < t->eng->stages.size(); ++i) if (t->eng->stages[i].name == "fpn.p6") t->trunk_last_stage = (int)i;
  if (t->trunk_last_stage < 0) { rs_set_error("trainer: engine has no fpn.p6 stage"); rc = RS_ERR_ARG; }
  if (!rc) rc = t->alloc((void**)&t->zeros, 16384 * 2);
  if (!rc) rc = t->alloc((void**)&t->zero_bias, 16384 * 4);
  if (!rc) rc = t->build_trunk_backward();
  if (!rc) rc = t->build_rpn_training();
  if (!rc) rc = t->build_box_training();
  if (!rc) rc = t->build_mask_training();
  if (!rc) {
    // the three loss stages run on the chain stream, one after the other; each kind has its own slots and counter
    const int SDm = 2 * spec->mask_pooler_resolution;
    const int caps[3] = {batch * (cdiv(t->A_total, 256) + 8), cdiv((long long)batch * rs_trainer::PC, 256) + 1,
                         cdiv((long long)batch * rs_trainer::MEI * SDm * SDm, 256) + 1};
    for (int k = 0; k < 3 && !rc; ++k) {
      t->loss_scratch[k].cap = caps[k];
      rc = t->alloc((void**)&t->loss_scratch[k].partial, (size_t)2 * caps[k] * 4);
      if (!rc) rc = t->alloc((void**)&t->loss_scratch[k].counter, 16);
    }
  }
  if (!rc) rc = t->alloc((void**)&t->master, t->n_params * 4);
  if (!rc) rc = t->alloc((void**)&t->grad, t->n_params * 4);
  if (!rc) rc = t->alloc((void**)&t->mom, t->n_params * 4);
  if (!rc) rc = t->alloc((void**)&t->partial, t->partial_floats * 4);
  if (!rc) {
    // master <- blob (.m32 weights, trainable biases from .b)
    for (const TrainLayer& L : t->layers) {
      const BlobEntry* m = t->eng->find(L.name + (L.bias_tile > 1 ? ".m32T" : ".m32"));
      if (!m || hipMemcpyAsync(t->master + L.w_off, m->dev, (size_t)L.Cout * L.Kpad * 4, hipMemcpyDeviceToDevice, t->stream) != hipSuccess) { rc = RS_ERR_HIP; break; }
      if (L.b_off != (size_t)-1 &&
          hipMemcpyAsync(t->master + L.b_off, L.b_fwd, (size_t)L.Cout * 4, hipMemcpyDeviceToDevice, t->stream) != hipSuccess) { rc = RS_ERR_HIP; break; }
      t->reg("g:" + L.name + ".w", t->grad + L.w_off, DT_F32, {L.Cout, L.Kpad}, 0);
      t->reg("m:" + L.name + ".w", t->master + L.w_off, DT_F32, {L.Cout, L.Kpad}, 0);
      if (L.b_off != (size_t)-1) {
        t->reg("g:" + L.name + ".b", t->grad + L.b_off, DT_F32, {L.Cout}, 0);
        t->reg("m:" + L.name + ".b", t->master + L.b_off, DT_F32, {L.Cout}, 0);
      }
    }
    if (rc) rs_set_error("trainer: copying master weights failed");
  }
  if (!rc) rc = t->fold_all();
  if (!rc) rc = t->build_buckets();
  if (!rc && hipStreamSynchronize(t->stream) != hipSuccess) { rs_set_error("trainer: sync failed"); rc = RS_ERR_HIP; }
  if (rc) { rs_trainer_destroy(t); return rc; }
  *out = t;
  return RS_OK;
}

void rs_trainer_destroy(rs_trainer* t) {
  if (!t) return;
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  if (t->side) { (void)hipStreamSynchronize(t->side); (void)hipStreamDestroy(t->side); }
  if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
  if (t->ev_dp32) (void)hipEventDestroy(t->ev_dp32);
  if (t->ev_rpn_targets) (void)hipEventDestroy(t->ev_rpn_targets);
  if (t->copy) { (void)hipStreamSynchronize(t->copy); (void)hipStreamDestroy(t->copy); }
  if (t->ev_rois) (void)hipEventDestroy(t->ev_rois);
  if (t->ev_targets) (void)hipEventDestroy(t->ev_targets);
  if (t->ev_polys) (void)hipEventDestroy(t->ev_polys);
  if (t->mt_pinned) (void)hipHostFree(t->mt_pinned);
  if (t->m_targets_pinned) (void)hipHostFree(t->m_targets_pinned);
  if (t->h_boxes) (void)hipHostFree(t->h_boxes);
  if (t->h_gti) (void)hipHostFree(t->h_gti);
  if (t->h_cnt) (void)hipHostFree(t->h_cnt);
  if (t->ev_join) (void)hipEventDestroy(t->ev_join);
  if (t->ev_foreign) (void)hipEventDestroy(t->ev_foreign);
  for (auto& b : t->buckets) { if (b.ev_main) (void)hipEventDestroy(b.ev_main); if (b.ev_side) (void)hipEventDestroy(b.ev_side); }
  for (auto& pr : t->pev) { if (pr.first) (void)hipEventDestroy(pr.first); if (pr.second) (void)hipEventDestroy(pr.second); }
  for (void* p : t->allocs) (void)hipFree(p);
  if (t->eng) rs_engine_destroy(t->eng);
  delete t;
}

rs_engine* rs_trainer_engine(rs_trainer* t) { return t ? t->eng : nullptr; }

// forward of the trunk (preprocess .. fpn.p6) on tiles resident in the engine's input buffer
int rs_trainer_forward_trunk(rs_trainer* t, const uint8_t* tiles_dev, int n) {
  RS_CHECK(t && tiles_dev && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  rs_engine* e = t->eng;
  { int rc = t->join_side(); if (rc) return rc; }          // the previous step's weight gradients read the activations overwritten here
  if (tiles_dev != e->tiles_dev)
    RS_HIP(hipMemcpyAsync(e->tiles_dev, tiles_dev, (size_t)n * e->tile_h * e->tile_w * e->tile_c, hipMemcpyDeviceToDevice, t->stream));
  for (int i = 0; i <= t->trunk_last_stage; ++i) {
    int rc = t->run_stage(e->stages[i], n, t->stream);
    if (rc) return rc;
  }
  t->rpn_forward_done = false;
  return RS_OK;
}

// Resized size of every image of the coming batches inside the trainer's canvas (n = 0: all fill it).  The preprocess stage then
// resizes image i to new_h[i] x new_w[i] (its own Pillow tables), leaves zeros beyond, and the proposals of image i are clipped to
// that size -- DatasetMapper's per-image ResizeShortestEdge draw + ImageList.from_tensors + Instances.image_size.
int rs_trainer_set_image_sizes(rs_trainer* t, const int32_t* new_h, const int32_t* new_w, int n) {
  RS_CHECK(t && n >= 0 && (n == 0 || (new_h && new_w)), RS_ERR_ARG, "bad argument");
  { int rc = t->join_side(); if (rc) return rc; }
  RS_HIP(hipStreamSynchronize(t->stream));            // the size table is read by kernels of the step in flight
  return t->eng->set_image_sizes(new_h, new_w, n);
}

// trunk backward from the current contents of d:p2..d:p6 into the flat gradient buffer
int rs_trainer_backward_trunk(rs_trainer* t, int n) {
  RS_CHECK(t && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  for (auto& c : t->clear_list) RS_HIP(hipMemsetAsync(c.first, 0, c.second, t->stream));
  { int rc = t->run_list(t->bwd, n); if (rc) return rc; }
  return RS_OK;
}

// ground truth of the batch: boxes in NETWORK-INPUT pixels [n][cap][4], classes [n][cap], counts [n] (host pointers).
// The classes of the counted boxes (j < gt_count[i]) are VALIDATED: one outside [0, NUM_CLASSES) is RS_ERR_ARG and nothing is
// copied (detectron2 fails in cross_entropy on such a target; the loss kernels would drop the RoI from loss_cls while still counting
// it, and the mask loss would train a padding channel of predictor16).  The padding slots beyond gt_count[i] are not looked at.
int rs_trainer_set_targets(rs_trainer* t, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_count, int n, int cap) {
  RS_CHECK(t && gt_boxes && gt_classes && gt_count && n >= 1 && n <= t->N && cap >= 1 && cap <= rs_trainer::GT_CAP, RS_ERR_ARG, "bad argument (at most %d boxes per image)", rs_trainer::GT_CAP);
  const int K = t->eng->spec.num_classes;
  for (int i = 0; i < n; ++i) {
    RS_CHECK(gt_count[i] >= 0 && gt_count[i] <= cap, RS_ERR_ARG, "gt_count[%d] = %d", i, gt_count[i]);
    for (int j = 0; j < gt_count[i]; ++j) {
      const int c = gt_classes[(size_t)i * cap + j];
      RS_CHECK(c >= 0 && c < K, RS_ERR_ARG, "image %d, box %d: ground-truth class %d outside [0, %d)", i, j, c, K);
    }
  }
  for (int i = 0; i < n; ++i) {
    RS_HIP(hipMemcpyAsync(t->gt_boxes + (size_t)i * rs_trainer::GT_CAP * 4, gt_boxes + (size_t)i * cap * 4, (size_t)cap * 16, hipMemcpyHostToDevice, t->stream));
    RS_HIP(hipMemcpyAsync(t->gt_classes + (size_t)i * rs_trainer::GT_CAP, gt_classes + (size_t)i * cap, (size_t)cap * 4, hipMemcpyHostToDevice, t->stream));
  }
  RS_HIP(hipMemcpyAsync(t->gt_count, gt_count, (size_t)n * 4, hipMemcpyHostToDevice, t->stream));
  RS_HIP(hipStreamSynchronize(t->stream));
  t->mt_set = false;                     // the pool holds the previous batch's polygons
  return RS_OK;
}

// Ground-truth polygons of the batch for mask targets rasterised on the device: the flat layout of rs_rasterize_entries (polygon q =
// poly_len[q] doubles at polys + poly_off[q], instance g owns polygons inst_first[g] .. inst_first[g+1]-1) plus image_first[n + 1], the
// first instance of every image (instance of image i's gt j = image_first[i] + j).  Coordinates in network-input pixels.  Packed into
// pinned staging and uploaded on the trainer's stream without a host wait; the staging buffer is guarded by an event like the
// targets' own.  A batch beyond the pool (rs_trainer: MT_POLYS_PER_IMAGE, MT_DOUBLES_PER_IMAGE) returns RS_POLYGONS_DO_NOT_FIT, copies
// nothing and leaves the trainer as it was: that step takes rs_trainer_fetch_rois + rs_trainer_mask_backward.
int rs_trainer_set_polygons(rs_trainer* t, const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first,
                            const int32_t* image_first, int n) {
  RS_CHECK(t && n >= 1 && n <= t->N && !t->mask_bwd.empty(), RS_ERR_ARG, "bad argument / MASK_ON false");
  RS_CHECK(2 * t->eng->spec.mask_pooler_resolution <= MT_MAX_SIDE, RS_ERR_UNSUPPORTED, "device mask targets: mask side above %d", MT_MAX_SIDE);
  RS_CHECK(image_first && image_first[0] == 0, RS_ERR_ARG, "image_first must start at 0");
  for (int i = 0; i < n; ++i) RS_CHECK(image_first[i + 1] >= image_first[i], RS_ERR_ARG, "image_first decreases at image %d", i);
  t->mt_set = false;
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, image_first[n], n, &L); if (rc) return rc; }
  const size_t cap_poly = (size_t)t->N * rs_trainer::MT_POLYS_PER_IMAGE, cap_dbl = (size_t)t->N * rs_trainer::MT_DOUBLES_PER_IMAGE;
  const size_t cap_inst = (size_t)t->N * rs_trainer::GT_CAP;
  if ((size_t)L.n_poly > cap_poly || L.n_doubles > cap_dbl || (size_t)L.n_inst > cap_inst) {
    rs_set_error("trainer: %d polygons / %zu doubles / %d instances do not fit the device pool (%zu / %zu / %zu)", L.n_poly, L.n_doubles,
                 L.n_inst, cap_poly, cap_dbl, cap_inst);
    return RS_POLYGONS_DO_NOT_FIT;
  }
  if (!t->mt_pool) {
    const size_t bytes = 4 * ((size_t)t->N + 1 + cap_inst + 1 + 2 * cap_poly) + 8 + 8 * cap_dbl;
    if (!t->ev_polys) RS_HIP(hipEventCreateWithFlags(&t->ev_polys, hipEventDisableTiming));
    if (!t->mt_pinned) RS_HIP(hipHostMalloc((void**)&t->mt_pinned, bytes, hipHostMallocDefault));
    { int rc = t->alloc((void**)&t->mt_pool, bytes); if (rc) return rc; }
  } else {
    RS_HIP(hipEventSynchronize(t->ev_polys));      // the previous upload has left the staging buffer
  }
  mt_pack(t->mt_pinned, L, polys, poly_off, poly_len, inst_first, image_first);
  RS_HIP(hipMemcpyAsync(t->mt_pool, t->mt_pinned, L.bytes, hipMemcpyHostToDevice, t->stream));
  RS_HIP(hipEventRecord(t->ev_polys, t->stream));
  t->mt_layout = L;
  t->mt_n = n;
  t->mt_set = true;
  return RS_OK;
}

// The RPN's training targets of the coming step (anchor Matcher + label subsampling, [EXT d2: modeling/proposal_generator/rpn.py
// label_and_sample_anchors]) on the SIDE stream, ahead of the forward pass: they read the ground truth (rs_trainer_set_targets) and the seed only.
// Call after rs_trainer_set_targets and before rs_trainer_forward_trunk; the rs_trainer_rpn_step of the same seed then waits for them instead of
// computing them on the chain (0.9 ms of single-workgroup-per-image kernels at batch 8).  Without a side stream, or with another seed later, the
// step computes them itself as before -- same kernels, same seed, same bits.
int rs_trainer_rpn_targets_async(rs_trainer* t, int n, uint32_t seed) {
  RS_CHECK(t && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  t->rpn_targets_ready = false;
  if (!t->side) return RS_OK;
  { int rc = t->join_side(); if (rc) return rc; }           // the previous step's side-stream work is ordered before the chain from here on
  if (!t->ev_rpn_targets) RS_HIP(hipEventCreateWithFlags(&t->ev_rpn_targets, hipEventDisableTiming));
  RS_HIP(hipEventRecord(t->ev_fork, t->stream));            // the previous step's rpn.loss (reader of the label buffers) is behind this point
  RS_HIP(hipStreamWaitEvent(t->side, t->ev_fork, 0));
  MatchParams m;
  memset(&m, 0, sizeof m);
  m.boxes = t->anchors; m.gt = t->gt_boxes; m.gt_count = t->gt_count; m.matched = t->rpn_matched; m.labels = t->rpn_labels;
  m.gt_best = t->gt_best; m.n_boxes = t->A_total; m.gt_cap = rs_trainer::GT_CAP;
  m.t_lo = 0.3f; m.t_hi = 0.7f; m.lbl_lo = 0; m.lbl_mid = -1; m.lbl_hi = 1;          // R:237-243
  { int rc = launch_match(m, n, t->side); if (rc) return rc; }
  SubsampleParams q;
  memset(&q, 0, sizeof q);
  q.labels = t->rpn_labels; q.n = t->A_total; q.num_samples = t->rpn_batch; q.positive_fraction = t->rpn_pos_frac; q.bg_label = 0; q.rpn_mode = 1;
  q.seed = seed * 2654435761u + 17u;
  { int rc = launch_subsample(q, n, t->side); if (rc) return rc; }
  RS_HIP(hipEventRecord(t->ev_rpn_targets, t->side));
  t->rpn_targets_seed = seed;
  t->rpn_targets_ready = true;
  return RS_OK;
}

// RPN head forward on the current FPN maps, targets + losses, head backward into d:p2..d:p6 (losses[0..1] accumulate).
// external_labels = 1: keep the labels / matches the caller wrote into "rpn_labels" / "rpn_matched" (parity tests).
int rs_trainer_rpn_step(rs_trainer* t, int n, uint32_t seed, int external_labels) {
  RS_CHECK(t && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  rs_engine* e = t->eng;
  if (!t->rpn_forward_done) {
    for (int i = t->rpn_first_stage; i <= t->rpn_last_stage; ++i) {
      int rc = t->run_stage(e->stages[i], n, t->stream);
      if (rc) return rc;
    }
  }
  t->rpn_forward_done = false;
  t->seed = seed;
  t->external_rpn_labels = external_labels != 0;
  if (!t->roi_grads_valid) {           // stand-alone RPN step: no RoI-head gradients to add, fresh loss accumulators
    RS_HIP(hipMemsetAsync(t->losses, 0, 8 * 4, t->stream));
    if (t->train_stats_on) RS_HIP(hipMemsetAsync(t->train_stats, 0, TS_TABLE * 4, t->stream));
    for (int l = 0; l < 4; ++l) if (t->dP32[l]) RS_HIP(hipMemsetAsync(t->dP32[l], 0, t->dP32_bytes[l], t->stream));
  }
  t->roi_grads_valid = false;
  { int rc = t->run_list(t->rpn_bwd, n); if (rc) return rc; }
  { int rc = t->run_stats(t->ts_rpn, n); if (rc) return rc; }      // behind every rpn.loss*: the labels are final
  return t->record_bucket(0);     // box / mask / RPN head gradients: rs_trainer_rpn_step is the last of the head steps
}

// RoI box head of the training forward + FastRCNNOutputLayers.losses + its backward.  Needs the RPN head outputs of the
// current batch (rs_trainer_rpn_forward).  Leaves loss_cls / loss_box_reg in "losses"[2..3] and the RoIAlign gradients in
// the fp32 maps "d32:p2".."d32:p5", which the following rs_trainer_rpn_step adds to the RPN's input gradient.
int rs_trainer_roi_step(rs_trainer* t, int n, uint32_t seed) {
  RS_CHECK(t && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  rs_engine* e = t->eng;
  hipStream_t s = t->stream;
  RS_HIP(hipMemsetAsync(t->losses, 0, 8 * 4, s));
  if (t->train_stats_on) RS_HIP(hipMemsetAsync(t->train_stats, 0, TS_TABLE * 4, s));
  for (int l = 0; l < 4; ++l) RS_HIP(hipMemsetAsync(t->dP32[l], 0, t->dP32_bytes[l], s));
  int rc;
  // proposals (detached): top PRE_NMS_TOPK_TRAIN per level, NMS, top POST_NMS_TOPK_TRAIN per image
  t->t_rp.N = n;
  t->t_rp.topk = t->rpn_pre_topk_train;
  t->t_merge.post_topk = t->rpn_post_topk_train < rs_trainer::PC ? t->rpn_post_topk_train : rs_trainer::PC;
  if ((rc = launch_rpn_select(t->t_rp, s))) return rc;
  if ((rc = launch_nms(t->t_nms, n * t->t_rp.L, s))) return rc;
  if ((rc = launch_rpn_merge(t->t_merge, n, s))) return rc;
  // label_and_sample_proposals
  if ((rc = launch_roi_candidates(t->rsp, n, s))) return rc;
  MatchParams m;
  memset(&m, 0, sizeof m);
  m.boxes = t->rsp.cand_boxes; m.per_image_boxes = 1; m.box_count = t->rsp.cand_count; m.gt = t->gt_boxes; m.gt_count = t->gt_count;
  m.matched = t->rsp.matched; m.labels = t->rsp.labels; m.n_boxes = rs_trainer::CAND_CAP; m.gt_cap = rs_trainer::GT_CAP;
  m.t_lo = 0.5f; m.t_hi = 0.5f; m.lbl_lo = 0; m.lbl_mid = 1; m.lbl_hi = 1;                                              // R:184-188
  if ((rc = launch_match(m, n, s))) return rc;
  if ((rc = launch_roi_classes(t->rsp, n, s))) return rc;
  SubsampleParams q;
  memset(&q, 0, sizeof q);
  q.labels = t->rsp.labels; q.sampled = t->roi_sampled; q.sampled_count = t->roi_sampled_count; q.n = rs_trainer::CAND_CAP;
  q.num_samples = t->roi_batch; q.positive_fraction = t->roi_pos_frac; q.bg_label = e->spec.num_classes; q.rpn_mode = 0;
  q.seed = seed * 2246822519u + 101u;
  if ((rc = launch_subsample(q, n, s))) return rc;
  t->rsp.num_samples = t->roi_batch;
  if ((rc = launch_roi_gather(t->rsp, n, s))) return rc;
  if (t->ev_rois) RS_HIP(hipEventRecord(t->ev_rois, s));
  for (int i = t->box_first_stage; i <= t->box_last_stage; ++i) if ((rc = t->run_stage(e->stages[i], n, s))) return rc;      // box head forward
  if ((rc = t->run_list(t->roi_bwd, n))) return rc;
  if ((rc = t->run_stats(t->ts_box, n))) return rc;               // behind box.loss, on the chain stream
  t->roi_grads_valid = true;
  return RS_OK;
}

// Mask head of the training step, after rs_trainer_roi_step: forward on the sampled foreground RoIs (entry e = image-major,
// sampled-foreground order: "mask_slots"/"mask_total"), mask_rcnn_loss against `targets` (host, [n_entries][28*28] 0/1, from
// train_targets.rasterize_polygons_within_box on "roi_boxes"/"roi_gt_index"), backward into d32:p2..p5.  loss_mask -> "losses"[4].
int rs_trainer_mask_forward(rs_trainer* t, int n) {
  RS_CHECK(t && n >= 1 && n <= t->N && !t->mask_fwd.empty(), RS_ERR_ARG, "bad argument / MASK_ON false");
  for (Stage& st : t->mask_fwd) {
    int rc = t->run_stage(st, n, t->stream);
    if (rc) return rc;
  }
  return RS_OK;
}
int rs_trainer_mask_backward(rs_trainer* t, int n, const uint8_t* targets_host, int n_entries) {
  RS_CHECK(t && n >= 1 && n <= t->N && !t->mask_bwd.empty() && n_entries >= 0 && n_entries <= n * rs_trainer::MEI, RS_ERR_ARG, "bad argument");
  const int side = 2 * t->eng->spec.mask_pooler_resolution;
  if (n_entries > 0) {
    RS_CHECK(targets_host, RS_ERR_ARG, "null targets");
    RS_HIP(hipEventSynchronize(t->ev_targets));  // the previous step's upload has left the staging buffer
    memcpy(t->m_targets_pinned, targets_host, (size_t)n_entries * side * side);
    RS_HIP(hipMemcpyAsync(t->m_targets, t->m_targets_pinned, (size_t)n_entries * side * side, hipMemcpyHostToDevice, t->stream));
    RS_HIP(hipEventRecord(t->ev_targets, t->stream));
  }
  { int rc = t->run_list(t->mask_bwd, n); if (rc) return rc; }
  return t->run_stats(t->ts_mask, n);                              // behind mask.loss, on the chain stream
}

// rs_trainer_mask_backward with the targets rasterised on the device (mask_targets_kernel on the chain stream, behind mask.entries and
// the sampling): no read-back, no host wait, no upload.  Needs the batch's polygons (rs_trainer_set_polygons after rs_trainer_set_targets).
int rs_trainer_mask_backward_device(rs_trainer* t, int n) {
  RS_CHECK(t && n >= 1 && n <= t->N && !t->mask_bwd.empty(), RS_ERR_ARG, "bad argument / MASK_ON false");
  RS_CHECK(t->mt_set && t->mt_n == n, RS_ERR_ARG, "no polygons of this batch on the device: call rs_trainer_set_polygons after rs_trainer_set_targets");
  { int rc = t->run_stage(t->mt_stage, n, t->stream); if (rc) return rc; }
  { int rc = t->run_list(t->mask_bwd, n); if (rc) return rc; }
  return t->run_stats(t->ts_mask, n);
}

// The sampled RoIs of the current rs_trainer_roi_step for the host-side mask targets: "roi_boxes" [n][1024][4], "roi_gt_index"
// [n][1024], "roi_sampled_count" [n][2] -> host.  Waits only for the sampling (an event recorded inside rs_trainer_roi_step),
// on its own copy stream: the box head's forward / backward and the mask head's forward keep the GPU busy meanwhile.
int rs_trainer_fetch_rois(rs_trainer* t, int n, float* boxes_host, int32_t* gt_index_host, int32_t* counts_host) {
  RS_CHECK(t && n >= 1 && n <= t->N && boxes_host && gt_index_host && counts_host && t->copy && t->h_boxes, RS_ERR_ARG, "bad argument / MASK_ON false");
  const size_t PCn = (size_t)n * rs_trainer::PC;
  RS_HIP(hipStreamWaitEvent(t->copy, t->ev_rois, 0));
  RS_HIP(hipMemcpyAsync(t->h_boxes, t->rsp.out_boxes, PCn * 16, hipMemcpyDeviceToHost, t->copy));
  RS_HIP(hipMemcpyAsync(t->h_gti, t->rsp.out_gt_index, PCn * 4, hipMemcpyDeviceToHost, t->copy));
  RS_HIP(hipMemcpyAsync(t->h_cnt, t->roi_sampled_count, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, t->copy));
  RS_HIP(hipStreamSynchronize(t->copy));
  memcpy(boxes_host, t->h_boxes, PCn * 16);
  memcpy(gt_index_host, t->h_gti, PCn * 4);
  memcpy(counts_host, t->h_cnt, (size_t)n * 2 * 4);
  return RS_OK;
}

// RPN head forward only (conv + fused heads on p2..p6)
int rs_trainer_rpn_forward(rs_trainer* t, int n) {
  RS_CHECK(t && n >= 1 && n <= t->N, RS_ERR_ARG, "bad argument");
  for (int i = t->rpn_first_stage; i <= t->rpn_last_stage; ++i) {
    int rc = t->run_stage(t->eng->stages[i], n, t->stream);
    if (rc) return rc;
  }
  t->rpn_forward_done = true;
  return RS_OK;
}

int rs_trainer_set_rpn_topk(rs_trainer* t, int pre_nms_topk_train, int post_nms_topk_train) {
  RS_CHECK(t && pre_nms_topk_train >= 1 && pre_nms_topk_train <= 2048 && post_nms_topk_train >= 1, RS_ERR_ARG, "RPN top-k outside [1, 2048]");
  t->rpn_pre_topk_train = pre_nms_topk_train;
  t->rpn_post_topk_train = post_nms_topk_train;
  return RS_OK;
}

int rs_trainer_set_sampling(rs_trainer* t, int rpn_batch, float rpn_positive_fraction, int roi_batch, float roi_positive_fraction) {
  RS_CHECK(t && rpn_batch >= 1 && roi_batch >= 1 && roi_batch <= rs_trainer::PC, RS_ERR_ARG, "bad sampling sizes (RoI batch at most %d)", rs_trainer::PC);
  t->rpn_batch = rpn_batch; t->rpn_pos_frac = rpn_positive_fraction; t->roi_batch = roi_batch; t->roi_pos_frac = roi_positive_fraction;
  return RS_OK;
}

int rs_trainer_set_wgrad_mode(rs_trainer* t, int mode) {
  RS_CHECK(t, RS_ERR_ARG, "rs_trainer_set_wgrad_mode: null trainer");
  RS_CHECK(mode == 0 || mode == 1, RS_ERR_ARG, "rs_trainer_set_wgrad_mode: mode %d (0 = fp32 matrix cores, 1 = split operands)", mode);
  RS_CHECK(t->f32 || mode == 0, RS_ERR_UNSUPPORTED, "rs_trainer_set_wgrad_mode: split operands serve the fp32 trainer; this one is fp16 and already on the fp16 matrix cores");
  if (mode == 1 && !t->wgs_scratch) {
    int rc = t->alloc(&t->wgs_scratch, wgrad_split_scratch_bytes(t->wgs_dy_cap, t->wgs_x_cap));   // zero-filled on the chain stream
    if (rc) return rc;
    RS_HIP(hipStreamSynchronize(t->stream));     // ... before a side-stream stage reads its zero row
  }
  t->wgrad_mode = mode;
  return RS_OK;
}

// Mirrors rs_trainer_set_wgrad_mode for the input gradients of the add_dgrad stages.  The first switch to mode 1 allocates the dY plane
// scratch and the planes of every w_bwd; every switch to mode 1 splits the current w_bwd (a fold in mode 0 does not).
int rs_trainer_set_dgrad_mode(rs_trainer* t, int mode) {
  RS_CHECK(t, RS_ERR_ARG, "rs_trainer_set_dgrad_mode: null trainer");
  RS_CHECK(mode == 0 || mode == 1, RS_ERR_ARG, "rs_trainer_set_dgrad_mode: mode %d (0 = fp32 matrix cores, 1 = split operands)", mode);
  RS_CHECK(t->f32 || mode == 0, RS_ERR_UNSUPPORTED, "rs_trainer_set_dgrad_mode: split operands serve the fp32 trainer; this one is fp16 and already on the fp16 matrix cores");
  if (mode == 1 && !t->dgs_scratch) {
    std::vector<SplitRowsDesc> tab;
    unsigned rows = 0;
    for (TrainLayer& L : t->layers) {
      if (!L.x_stage || L.w_bwd_planes) continue;
      int rc = t->alloc((void**)&L.w_bwd_planes, (size_t)L.Cin * L.KpadT * 4);
      if (!rc) rc = t->alloc((void**)&L.w_bwd_inv, (size_t)L.Cin * 4);
      if (rc) return rc;
    }
    for (const TrainLayer& L : t->layers) {
      if (!L.x_stage) continue;
      tab.push_back(SplitRowsDesc{(const float*)L.w_bwd, L.w_bwd_planes, L.w_bwd_inv, L.Cin, L.KpadT, rows});
      rows += (unsigned)L.Cin;
    }
    RS_CHECK(!tab.empty(), RS_ERR_ARG, "rs_trainer_set_dgrad_mode: no layer has input-gradient weights");
    if (!t->dgs_table) { int rc = t->alloc((void**)&t->dgs_table, tab.size() * sizeof(SplitRowsDesc)); if (rc) return rc; }
    RS_HIP(hipMemcpyAsync(t->dgs_table, tab.data(), tab.size() * sizeof(SplitRowsDesc), hipMemcpyHostToDevice, t->stream));
    RS_HIP(hipStreamSynchronize(t->stream));      // tab is a local
    t->dgs_n = (int)tab.size(); t->dgs_rows = rows;
    int rc = t->alloc(&t->dgs_scratch, dgrad_split_scratch_bytes(t->dgs_cap));
    if (rc) return rc;
  }
  if (mode == 1) { int rc = t->split_w_bwd(); if (rc) return rc; }
  t->dgrad_mode = mode;
  return RS_OK;
}

// The forward product's mode lives in the forward engine (rs_engine::set_fwd_mode): the first switch to mode 1 allocates the X plane
// scratch and the planes of every served layer's weight; every switch to mode 1 splits all of them (a fold in mode 0 does not).
int rs_trainer_set_fwd_mode(rs_trainer* t, int mode) {
  RS_CHECK(t, RS_ERR_ARG, "rs_trainer_set_fwd_mode: null trainer");
  RS_CHECK(mode == 0 || mode == 1, RS_ERR_ARG, "rs_trainer_set_fwd_mode: mode %d (0 = fp32 matrix cores, 1 = split operands)", mode);
  RS_CHECK(t->f32 || mode == 0, RS_ERR_UNSUPPORTED, "rs_trainer_set_fwd_mode: split operands serve the fp32 trainer; this one is fp16 and already on the fp16 matrix cores");
  if (!t->f32) return RS_OK;
  return t->eng->set_fwd_mode(mode, t->folded_weights());
}

// Training diagnostics: the first switch-on allocates the table, names it and builds the three stages on the buffers the loss stages
// read; later calls only flip the flag, which is read when a step runs.
int rs_trainer_set_train_stats(rs_trainer* t, int on) {
  RS_CHECK(t, RS_ERR_ARG, "rs_trainer_set_train_stats: null trainer");
  RS_CHECK(on == 0 || on == 1, RS_ERR_ARG, "rs_trainer_set_train_stats: value %d (0 = off, 1 = on)", on);
  if (on && !t->train_stats) {
    const rs_spec& S = t->eng->spec;
    const int K = S.num_classes, SD = 2 * S.mask_pooler_resolution;
    const int pred_cs = (5 * K + 1 + 15) / 16 * 16;
    const bool mask = !t->mask_bwd.empty();
    // every counter is bounded by one of these products
    const long long lim = 1ll << 31;
    RS_CHECK((long long)t->N * t->A_total < lim && (long long)t->N * rs_trainer::PC < lim &&
             (!mask || (long long)t->N * rs_trainer::MEI * SD * SD < lim), RS_ERR_UNSUPPORTED,
             "rs_trainer_set_train_stats: a batch of %d lets a count reach 2^31 (%d anchors, %d RoI slots, %d x %d x %d mask pixels per image)",
             t->N, t->A_total, rs_trainer::PC, rs_trainer::MEI, SD, SD);
    RS_CHECK(K >= 1 && K <= TS_MAX_CLASSES, RS_ERR_UNSUPPORTED, "rs_trainer_set_train_stats: %d classes", K);
    const float* pred = nullptr;
    const float* logits = nullptr;
    for (const TensorInfo& ti : t->eng->tensors) if (ti.name == "box_pred") pred = (const float*)ti.p;
    for (const TensorInfo& ti : t->tensors) if (ti.name == "t:mask_logits") logits = (const float*)ti.p;
    RS_CHECK(pred && (!mask || logits), RS_ERR_ARG, "rs_trainer_set_train_stats: the loss stages' tensors are missing");
    int* table = nullptr;
    { int rc = t->alloc((void**)&table, TS_TABLE * 4); if (rc) return rc; }      // zero-filled on the chain stream
    rs_trainer* self = t;
    t->ts_box.name = "box.stats";
    t->ts_box.fn = [self, table, pred, K, pred_cs](int n, hipStream_t s) {
      BoxStatsParams q;
      memset(&q, 0, sizeof q);
      q.pred = pred; q.gt_classes = self->rsp.out_classes; q.sampled_counts = self->roi_sampled_count; q.out = table + TS_ROI;
      q.n_rois = n * rs_trainer::PC; q.K = K; q.cs = pred_cs; q.n_images = n;
      return launch_box_stats(q, s);
    };
    t->ts_mask.name = "mask.stats";
    t->ts_mask.fn = [self, table, logits, SD](int n, hipStream_t s) {
      MaskStatsParams q;
      memset(&q, 0, sizeof q);
      q.logits = logits; q.targets = self->m_targets; q.gt_classes = self->m_cls; q.n_masks_ptr = self->m_total; q.out = table + TS_MASK;
      q.n_masks = n * rs_trainer::MEI; q.S = SD; q.cs = 16;
      return launch_mask_stats(q, s);
    };
    t->ts_rpn.name = "rpn.stats";
    t->ts_rpn.fn = [self, table](int n, hipStream_t s) {
      LabelCountsParams q;
      memset(&q, 0, sizeof q);
      q.labels = self->rpn_labels; q.count = n * self->A_total; q.out = table + TS_RPN; q.images_out = table + TS_IMAGES; q.images = n;
      return launch_label_counts(q, s);
    };
    TensorInfo ti;
    ti.name = "train_stats"; ti.p = table; ti.dtype = DT_I32; ti.ndim = 1; ti.halo = 0;
    ti.dims[0] = TS_TABLE;
    ti.bytes = TS_TABLE * 4;
    t->named.push_back(ti);
    t->train_stats = table;
  }
  t->train_stats_on = on;
  return RS_OK;
}

// The solver of the following optimiser steps.  The first call cuts the flat buffers along the segment table, uploads the chunk table
// behind everything enqueued so far and registers "grad_norms" / "clip_coef"; later calls only replace the values, which are read when
// rs_trainer_apply_sgd runs.
int rs_trainer_set_solver(rs_trainer* t, const rs_solver* solver) {
  RS_CHECK(t, RS_ERR_ARG, "rs_trainer_set_solver: null trainer");
  { int rc = sgd_solver_check("rs_trainer_set_solver", solver); if (rc) return rc; }
  if (!t->sgd_plan.chunks) {
    const auto& segs = t->segment_table();
    std::vector<int64_t> off, cnt;
    std::vector<int32_t> flags;
    for (const auto& s : segs) { off.push_back((int64_t)s.off); cnt.push_back((int64_t)s.count); flags.push_back(s.bias ? SGD_SEG_BIAS : 0); }
    std::vector<SgdChunk> chunks;
    std::vector<int> seg_chunks;
    std::vector<uint8_t> host;
    { int rc = sgd_plan_cut("rs_trainer_set_solver", off.data(), cnt.data(), flags.data(), (int)segs.size(), (long long)t->n_params, &chunks, &seg_chunks); if (rc) return rc; }
    sgd_plan_pack(chunks, seg_chunks, &host);
    void* base = nullptr;
    { int rc = t->alloc(&base, sgd_plan_bytes((int)chunks.size(), (int)segs.size())); if (rc) return rc; }      // zero-filled on the chain stream
    RS_HIP(hipStreamSynchronize(t->stream));
    RS_HIP(hipMemcpy(base, host.data(), host.size(), hipMemcpyHostToDevice));
    t->sgd_plan = sgd_plan_place(base, (int)chunks.size(), (int)segs.size());
    t->reg("grad_norms", t->sgd_plan.norms, DT_F32, {(int64_t)segs.size()}, 0);
    t->reg("clip_coef", t->sgd_plan.coef, DT_F32, {(int64_t)segs.size()}, 0);
  }
  t->solver = *solver;
  t->solver_on = true;
  return RS_OK;
}
int rs_trainer_segment_count(rs_trainer* t) { return t ? (int)t->segment_table().size() : 0; }
int rs_trainer_segment_info(rs_trainer* t, int i, char* name_out, int64_t* offset, int64_t* count, int* is_bias) {
  RS_CHECK(t && i >= 0 && i < (int)t->segment_table().size(), RS_ERR_ARG, "segment index");
  const auto& s = t->segments[i];
  if (name_out) { strncpy(name_out, s.name.c_str(), 95); name_out[95] = 0; }
  if (offset) *offset = (int64_t)s.off;
  if (count) *count = (int64_t)s.count;
  if (is_bias) *is_bias = s.bias;
  return RS_OK;
}

int rs_trainer_sync(rs_trainer* t) {
  RS_CHECK(t, RS_ERR_ARG, "null trainer");
  { int rc = t->join_side(); if (rc) return rc; }
  RS_HIP(hipStreamSynchronize(t->stream));
  return RS_OK;
}

// one SGD-momentum step on every trainable tensor from the current gradient buffer, then refold the fp16 operands
int rs_trainer_apply_sgd(rs_trainer* t, float lr, float momentum, float weight_decay) {
  RS_CHECK(t, RS_ERR_ARG, "null trainer");
  const float inv_scale = 1.f / (t->loss_scale * t->grad_divisor);
  SgdHyper h;
  int norm_inf = 0;
  if (t->solver_on) {      // before anything is enqueued: Nesterov needs a momentum
    int rc = sgd_solver_hyper("rs_trainer_apply_sgd", t->solver, lr, momentum, weight_decay, inv_scale, &h, &norm_inf);
    if (rc) return rc;
  }
  int rc = t->join_side();
  if (rc) return rc;
  if (t->solver_on) {
    // the segmented step (sgd_rule.h).  A norm pass reads the whole gradient anyway and raises "grad_overflow" itself; without one the
    // separate check runs as below
    if (h.clip_type >= SGD_CLIP_NORM) rc = launch_grad_norms(t->sgd_plan, t->grad, h, norm_inf, t->overflow, t->stream);
    else rc = launch_grad_nonfinite(t->grad, (long long)t->n_params, t->overflow, t->stream);
    if (!rc) rc = launch_sgd_segments(t->sgd_plan, t->master, t->mom, t->grad, h, t->overflow, t->stream);
    if (rc) return rc;
    ++t->step_count;
    return t->fold_all();
  }
  // a gradient with inf / nan (fp16 loss scale too large for this batch) must not reach the weights: the step is skipped on the
  // device (no host round trip); the caller reads "grad_overflow" with the losses and lowers the scale (rs_trainer_set_loss_scale)
  rc = launch_grad_nonfinite(t->grad, (long long)t->n_params, t->overflow, t->stream);
  if (rc) return rc;
  // momentum starts at zero, so "first step" needs no special case (mu * 0 + g = g) -- and a skipped first step stays correct
  rc = launch_sgd_momentum(t->master, t->mom, t->grad, (long long)t->n_params, lr, momentum, weight_decay, 1.f / (t->loss_scale * t->grad_divisor),
                           0, t->stream, t->overflow);
  if (rc) return rc;
  ++t->step_count;
  return t->fold_all();
}

// fp16 loss scale of the NEXT rs_trainer_* step sequence (call it between rs_trainer_apply_sgd and the next forward: the
// gradient buffer carries the scale it was computed with)
int rs_trainer_set_loss_scale(rs_trainer* t, float loss_scale) {
  RS_CHECK(t && loss_scale > 0.f, RS_ERR_ARG, "bad loss scale");
  t->loss_scale = loss_scale;
  return RS_OK;
}

int rs_trainer_tensor(rs_trainer* t, const char* name, void** dev_ptr, int* dtype, int* ndim, int64_t dims[5], int* halo) {
  RS_CHECK(t && name, RS_ERR_ARG, "null argument");
  for (const TensorInfo& ti : t->tensors) {
    if (ti.name == name) {
      if (dev_ptr) *dev_ptr = ti.p;
      if (dtype) *dtype = ti.dtype;
      if (ndim) *ndim = ti.ndim;
      if (dims) for (int i = 0; i < 5; ++i) dims[i] = ti.dims[i];
      if (halo) *halo = ti.halo;
      return RS_OK;
    }
  }
  for (const TensorInfo& ti : t->named) {
    if (ti.name == name) {
      if (dev_ptr) *dev_ptr = ti.p;
      if (dtype) *dtype = ti.dtype;
      if (ndim) *ndim = ti.ndim;
      if (dims) for (int i = 0; i < 5; ++i) dims[i] = ti.dims[i];
      if (halo) *halo = ti.halo;
      return RS_OK;
    }
  }
  rs_set_error("trainer: no tensor named %s", name);
  return RS_ERR_ARG;
}
int rs_trainer_tensor_count(rs_trainer* t) { return t ? (int)t->tensors.size() : 0; }
int rs_trainer_tensor_name(rs_trainer* t, int i, char* name_out) {
  RS_CHECK(t && i >= 0 && i < (int)t->tensors.size() && name_out, RS_ERR_ARG, "tensor index");
  strncpy(name_out, t->tensors[i].name.c_str(), 95);
  name_out[95] = 0;
  return RS_OK;
}
// Multi-scale training (INPUT.MIN_SIZE_TRAIN "choice", R:31-38): one trainer per network-input geometry; before a step on
// `dst` the optimiser state of the trainer that ran the previous step is copied over (two device-to-device copies of the flat
// buffers) and dst's fp16 operands are refolded.
int rs_trainer_copy_state(rs_trainer* dst, rs_trainer* src) {
  RS_CHECK(dst && src && dst->freeze_at == src->freeze_at, RS_ERR_ARG, "trainers differ in MODEL.BACKBONE.FREEZE_AT (%d and %d)", dst ? dst->freeze_at : -1, src ? src->freeze_at : -1);
  RS_CHECK(dst->n_params == src->n_params && dst->layers.size() == src->layers.size(), RS_ERR_ARG, "trainers differ in their parameter layout");
  if (dst == src) return RS_OK;
  { int rc = src->join_side(); if (!rc) rc = dst->join_side(); if (rc) return rc; }
  RS_HIP(hipStreamSynchronize(src->stream));
  RS_HIP(hipMemcpyAsync(dst->master, src->master, dst->n_params * 4, hipMemcpyDeviceToDevice, dst->stream));
  RS_HIP(hipMemcpyAsync(dst->mom, src->mom, dst->n_params * 4, hipMemcpyDeviceToDevice, dst->stream));
  dst->step_count = src->step_count;
  // the solver travels with the state: the destination cuts its own (identical) table on first use
  if (src->solver_on) { int rc = rs_trainer_set_solver(dst, &src->solver); if (rc) return rc; }
  else dst->solver_on = false;
  // the forward mode travels with the state, as the input-gradient mode below: switched off at once, switched on behind the fold
  const bool fwd_on = dst->eng->fwd_mode != src->eng->fwd_mode && src->eng->fwd_mode == 1;
  if (dst->eng->fwd_mode != src->eng->fwd_mode && src->eng->fwd_mode == 0) { int rc = rs_trainer_set_fwd_mode(dst, 0); if (rc) return rc; }
  if (dst->dgrad_mode != src->dgrad_mode) {       // the input-gradient mode travels with the state (its switch-on splits after the fold below)
    if (src->dgrad_mode == 0) dst->dgrad_mode = 0;
    else {
      int rc = dst->fold_all();
      if (!rc) rc = rs_trainer_set_dgrad_mode(dst, src->dgrad_mode);
      if (!rc && fwd_on) rc = rs_trainer_set_fwd_mode(dst, 1);
      return rc;
    }
  }
  int rc = dst->fold_all();
  if (!rc && fwd_on) rc = rs_trainer_set_fwd_mode(dst, 1);
  return rc;
}

int rs_trainer_set_grad_divisor(rs_trainer* t, float d) {
  RS_CHECK(t && d > 0.f, RS_ERR_ARG, "bad divisor");
  t->grad_divisor = d;
  return RS_OK;
}
int rs_trainer_bucket_count(rs_trainer* t) { return t ? (int)t->buckets.size() : 0; }
int rs_trainer_bucket_info(rs_trainer* t, int i, char* name_out, int64_t* offset, int64_t* count) {
  RS_CHECK(t && i >= 0 && i < (int)t->buckets.size(), RS_ERR_ARG, "bucket index");
  if (name_out) { strncpy(name_out, t->buckets[i].name.c_str(), 95); name_out[95] = 0; }
  if (offset) *offset = (int64_t)t->buckets[i].off;
  if (count) *count = (int64_t)t->buckets[i].count;
  return RS_OK;
}
// device-side: everything enqueued on `stream` after this call runs behind bucket i's gradients of the current step
int rs_trainer_bucket_wait(rs_trainer* t, int i, void* stream) {
  RS_CHECK(t && i >= 0 && i < (int)t->buckets.size(), RS_ERR_ARG, "bucket index");
  RS_HIP(hipStreamWaitEvent((hipStream_t)stream, t->buckets[i].ev_main, 0));
  if (t->side) RS_HIP(hipStreamWaitEvent((hipStream_t)stream, t->buckets[i].ev_side, 0));
  return RS_OK;
}
// host-side: returns once bucket i's gradients of the current step are complete
int rs_trainer_bucket_sync(rs_trainer* t, int i) {
  RS_CHECK(t && i >= 0 && i < (int)t->buckets.size(), RS_ERR_ARG, "bucket index");
  RS_HIP(hipEventSynchronize(t->buckets[i].ev_main));
  if (t->side) RS_HIP(hipEventSynchronize(t->buckets[i].ev_side));
  return RS_OK;
}
// the trainer's chain stream waits for everything enqueued so far on `stream` (a collective's stream) -- call it before
// rs_trainer_apply_sgd
int rs_trainer_wait_stream(rs_trainer* t, void* stream) {
  RS_CHECK(t, RS_ERR_ARG, "null trainer");
  RS_HIP(hipEventRecord(t->ev_foreign, (hipStream_t)stream));
  RS_HIP(hipStreamWaitEvent(t->stream, t->ev_foreign, 0));
  return RS_OK;
}
// Per-stage timing of the training step (HIP events on the stream each stage runs on; concurrent streams overlap, so the per-stage
// times of a step add up to MORE than its wall time).  on = 1: clear the accumulators and time every following stage (up to 8192
// stage executions); 0: stop.  rs_trainer_stage_count resolves the outstanding events (synchronises both streams).
int rs_trainer_set_profiling(rs_trainer* t, int on) {
  RS_CHECK(t, RS_ERR_ARG, "null trainer");
  { int rc = t->resolve_profile(); if (rc) return rc; }
  if (t->all_stages.empty()) {
    for (int i = 0; i <= t->box_last_stage && i < (int)t->eng->stages.size(); ++i) t->all_stages.push_back(&t->eng->stages[i]);
    for (auto* l : {&t->roi_bwd, &t->mask_fwd, &t->mask_bwd, &t->rpn_bwd, &t->bwd})
      for (Stage& st : *l) t->all_stages.push_back(&st);
  }
  if (t->mt_pool && !t->mt_listed) { t->all_stages.push_back(&t->mt_stage); t->mt_listed = true; }   // last: the other indices stay
  if (t->train_stats && !t->ts_listed) {
    t->all_stages.push_back(&t->ts_box);
    if (!t->mask_bwd.empty()) t->all_stages.push_back(&t->ts_mask);
    t->all_stages.push_back(&t->ts_rpn);
    t->ts_listed = true;
  }
  if (on) {
    for (Stage* st : t->all_stages) { st->ms_total = 0; st->calls = 0; st->last_flops = 0; }
    if (t->pev.empty()) {
      t->pev.resize(8192); t->pev_stage.resize(8192); t->pev_n.resize(8192);
      for (auto& pr : t->pev) { RS_HIP(hipEventCreate(&pr.first)); RS_HIP(hipEventCreate(&pr.second)); }
    }
  }
  t->profiling = on ? 1 : 0;
  return RS_OK;
}
int rs_trainer_stage_count(rs_trainer* t) {
  if (!t || t->resolve_profile() != RS_OK) return 0;
  return (int)t->all_stages.size();
}
int rs_trainer_stage_info(rs_trainer* t, int i, char* name_out, double* ms_total, int* calls, double* flops, int* on_side_stream) {
  RS_CHECK(t && i >= 0 && i < (int)t->all_stages.size(), RS_ERR_ARG, "stage index");
  const Stage& st = *t->all_stages[i];
  if (name_out) { strncpy(name_out, st.name.c_str(), 95); name_out[95] = 0; }
  if (ms_total) *ms_total = st.ms_total;
  if (calls) *calls = st.calls;
  if (flops) *flops = st.last_flops;
  if (on_side_stream) *on_side_stream = (st.grad_side && t->side) ? 1 : 0;
  return RS_OK;
}

// Operator-level entry of mask_targets_kernel: the arguments of rs_rasterize_entries (host pointers) without `threads`; packs and
// uploads the polygons, rasterises the n_entries explicit (instance, box) pairs on the device and copies the masks back.  An entry
// whose instance is outside [0, n_inst) comes back all zero.
int rs_op_mask_targets(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst,
                       const int32_t* entry_inst, const float* boxes, int n_entries, int mask_size, uint8_t* out) {
  if (n_entries == 0) return RS_OK;
  RS_CHECK(entry_inst && boxes && out && n_inst > 0 && n_entries > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(mask_size >= 2 && mask_size <= MT_MAX_SIDE && mask_size % 2 == 0, RS_ERR_UNSUPPORTED, "mask_targets: even mask side up to %d", MT_MAX_SIDE);
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, n_inst, 0, &L); if (rc) return rc; }
  RS_CHECK(L.n_doubles <= (size_t)MT_MAX_DOUBLES, RS_ERR_UNSUPPORTED, "mask_targets: more than %d doubles of polygons", MT_MAX_DOUBLES);
  std::vector<uint8_t> host(L.bytes);
  const int32_t zero = 0;
  mt_pack(host.data(), L, polys, poly_off, poly_len, inst_first, &zero);
  const size_t SS = (size_t)mask_size * mask_size;
  uint8_t* pool = nullptr; float* bx = nullptr; int* ei = nullptr; uint8_t* m = nullptr;
  int rc = RS_OK;
  if (hipMalloc((void**)&pool, L.bytes) != hipSuccess || hipMalloc((void**)&bx, (size_t)n_entries * 16) != hipSuccess ||
      hipMalloc((void**)&ei, (size_t)n_entries * 4) != hipSuccess || hipMalloc((void**)&m, (size_t)n_entries * SS) != hipSuccess ||
      hipMemcpy(pool, host.data(), L.bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(bx, boxes, (size_t)n_entries * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(ei, entry_inst, (size_t)n_entries * 4, hipMemcpyHostToDevice) != hipSuccess) {
    rs_set_error("mask_targets: device buffers"); rc = RS_ERR_HIP;
  }
  if (!rc) {
    MaskTargetsParams q;
    memset(&q, 0, sizeof q);
    q.boxes = bx; q.gt_index = ei; q.inst_first = (const int*)(pool + L.o_inst); q.poly_off = (const int*)(pool + L.o_off);
    q.poly_len = (const int*)(pool + L.o_len); q.polys = (const double*)(pool + L.o_xy);
    q.out = m; q.n_entries = n_entries; q.n_inst = n_inst; q.S = mask_size;
    rc = launch_mask_targets(q, nullptr);
    if (!rc && hipMemcpy(out, m, (size_t)n_entries * SS, hipMemcpyDeviceToHost) != hipSuccess) { rs_set_error("mask_targets: read-back"); rc = RS_ERR_HIP; }
  }
  (void)hipFree(pool); (void)hipFree(bx); (void)hipFree(ei); (void)hipFree(m);
  return rc;
}

void* rs_trainer_master_buffer(rs_trainer* t) { return t ? (void*)t->master : nullptr; }
int64_t rs_trainer_param_count(rs_trainer* t) { return t ? (int64_t)t->n_params : 0; }
void* rs_trainer_grad_buffer(rs_trainer* t) { return t ? (void*)t->grad : nullptr; }

}  // extern "C"
