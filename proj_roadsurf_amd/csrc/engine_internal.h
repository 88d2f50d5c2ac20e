// Internal to the host units engine.hip, ops.hip and trainer.hip (nothing else includes it): the engine object with its tensor,
// stage and blob types, as the trainer drives them directly.  The C ABI is include/rs_engine.h.
#pragma once
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/rs_engine.h"
#include "detect.h"
#include "polygonize.h"

// DT_SPLIT16: an activation of the split-operand mode -- two fp16 planes of the registered shape back to back (hi, then lo); value = hi + lo
enum { DT_F16 = 1, DT_F32 = 2, DT_I32 = 3, DT_U8 = 4, DT_SPLIT16 = 5 };
inline size_t dt_size(int dt) { return (dt == DT_F16 || dt == DT_SPLIT16) ? 2 : (dt == DT_U8 ? 1 : 4); }

struct TensorInfo {
  std::string name;
  void* p = nullptr;
  int dtype = 0, ndim = 0, halo = 0;
  int64_t dims[5] = {1, 1, 1, 1, 1};
  size_t bytes = 0;
};

struct Act {   // NHWC fp16 activation with halo
  half_t* p = nullptr;
  long long lo = 0;   // split-operand mode: element offset of the lo plane behind p (0 = single plane)
  int N = 0, H = 0, W = 0, C = 0, pad = 0;
  int Hp() const { return H + 2 * pad; }
  int Wp() const { return W + 2 * pad; }
};

struct Stage {
  std::string name;
  std::function<int(int, hipStream_t)> fn;
  double flops_per_image = 0, bytes_per_image = 0;   // algorithmic, per tile (0 = n/a)
  double ms_total = 0;
  int calls = 0;
  double last_flops = 0, last_bytes = 0;
  int variant = -2;      // conv tile variant of the last call (-2 = not a conv stage)
  bool narrow = false;   // latency-bound detection glue (few workgroups): runs on the engine's side stream
  bool grad_side = false;   // trainer: weight / bias gradient, off the input-gradient chain (may run on the trainer's side stream)
  int bucket = -1;          // trainer: gradient bucket this stage writes into (rs_trainer::buckets), -1 = none
  int phase = 0;         // 0 = preprocess..RPN proposals, 1 = box head..detections, 2 = mask head + paste
  hipEvent_t handoff = nullptr;   // recorded on the previous stage's stream when this stage switches streams
};

struct BlobEntry { const void* host; void* dev; int dtype; int ndim; int64_t dims[4]; size_t nbytes; };

// =================================================================================== engine
struct rs_engine {
  rs_spec spec;
  int device = 0;
  hipStream_t stream = nullptr;         // "wide" stream: every kernel that fills the chip (may be shared between engines)
  bool own_stream = false;
  hipStream_t copy_stream = nullptr;    // device-to-host result copies (rs_engine_fetch_async), overlapping the next batch
  hipEvent_t ev_results = nullptr;      // recorded on `stream` when a forward's results are complete
  hipEvent_t ev_copied = nullptr;       // recorded on `copy_stream` after the last result copy; the next forward's box head waits for it
  bool copy_pending = false;
  hipStream_t narrow = nullptr;         // side stream for the latency-bound glue kernels (null = everything on `stream`)
  bool on_narrow = false;               // which stream the most recently enqueued stage went to
  hipEvent_t ev_join = nullptr;         // narrow -> wide join at the end of a forward that ends on the side stream
  bool cur_record = false;              // profiling decision of the forward in flight (taken at phase 0)
  int max_batch = 0, tile_h = 0, tile_w = 0, tile_c = 0;
  int net_h = 0, net_w = 0, pad_h = 0, pad_w = 0;
  int use_glds = 1;    // -1 = fp32 validation path (launch_conv forwards to launch_conv_f32)
  bool f32 = false;    // rs_spec.precision == 1: activations and weights are float
  bool split = false;  // rs_spec.precision == 2: split-operand mode -- activations and weights as hi + lo fp16 planes, three MFMA passes (common.h ConvParams::split)
  int profiling = 0;   // 0 off, 1 = events + host sync per stage, 2 = events only (resolved later)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;   // mode 2
  std::vector<int> ev_stage;
  std::vector<int> ev_batch;
  size_t ev_used = 0;
  int resolve_profile();

  void* blob_dev = nullptr;
  std::map<std::string, BlobEntry> blob;
  std::vector<void*> allocs;
  std::vector<TensorInfo> tensors;
  std::vector<Stage> stages;

  uint8_t* tiles_dev = nullptr;
  // per-image resized sizes inside the net_h x net_w canvas (training: INPUT.MIN_SIZE_TRAIN drawn per image, the batch padded to the
  // largest -- [EXT d2: data/dataset_mapper.py, structures/image_list.py]); empty = every image fills the canvas
  struct ResizeTab { int* b = nullptr; int* k = nullptr; int ks = 0; };
  std::map<int, ResizeTab> tab_h, tab_v;   // by output size
  std::vector<int> img_new_h, img_new_w;
  float* img_hw_dev = nullptr;             // [max_batch][2] clip size of the proposals per image (h, w)
  int resize_tab(int in_size, int out_size, std::map<int, ResizeTab>& cache, ResizeTab* out);
  int set_image_sizes(const int32_t* new_h, const int32_t* new_w, int n);
  // results (device)
  int* det_count = nullptr;
  float* det_boxes = nullptr;
  float* det_boxes_net = nullptr;
  float* det_scores = nullptr;
  int* det_classes = nullptr;
  uint8_t* masks = nullptr;
  float* mask_probs = nullptr;
  int D = 0;
  // mask crops for the host (rs_engine_fetch_crops_*): table + compacted data on the device, byte count read back pinned
  int* crop_rects = nullptr;
  unsigned int* crop_offsets = nullptr;
  unsigned long long* crop_total = nullptr;
  uint8_t* crop_data = nullptr;
  unsigned long long* h_crop_total = nullptr;   // pinned
  hipEvent_t ev_crop_hdr = nullptr;
  // polygons for the host (rs_engine_fetch_polygons_*): allocated on the first call, an engine that never asks keeps none of it
  PolyParams poly;                              // scratch + compacted tables on the device
  bool poly_ready = false;
  int* h_poly_totals = nullptr;                 // pinned [4]
  hipEvent_t ev_poly_hdr = nullptr;

  // validation counts for the host (rs_engine_fetch_eval_*): allocated on the first call, like the polygons' buffers
  uint8_t* eval_pool = nullptr;                 // device: the batch's ground-truth polygons (polygon_pool.h)
  uint8_t* eval_pinned = nullptr;               // pinned staging of the pool
  size_t eval_pool_bytes = 0;
  uint8_t* eval_gt_masks = nullptr;             // [max_batch * RS_EVAL_GT_CAP][tile_h][ceil(tile_w / 8)]
  int *eval_inter = nullptr, *eval_det_area = nullptr, *eval_gt_area = nullptr;
  hipEvent_t ev_eval_upload = nullptr;          // recorded behind the pool's upload: the staging may be packed again after it
  bool eval_upload_pending = false;
  // match tables (rs_engine_fetch_eval_match_*): allocated on the first call that asks for them
  uint8_t* match_pinned = nullptr;              // pinned staging: gt boxes [max_batch * RS_EVAL_GT_CAP][4] doubles, then their classes
  double* match_gt_boxes = nullptr;             // device (one allocation with the classes behind the boxes)
  int* match_order = nullptr;                   // device: the five tables of coco_match.h behind each other, see ensure_match_buffers
  int *match_class_first = nullptr, *match_gt_per_class = nullptr, *match_npig = nullptr;
  uint32_t *match_matched = nullptr, *match_ignored = nullptr;
  int ensure_match_buffers();
  // vote tables (rs_engine_fetch_votes_*, road_vote.h): allocated on the first call
  double* vote_wscore = nullptr;                // device: wscore [max_batch][RS_EVAL_GT_CAP][K], then wfrac of the same shape
  int* vote_pairs = nullptr;
  size_t vote_cells = 0;
  int ensure_vote_buffers();
  // the sweep's tables (rs_engine_fetch_vote_sweep_*): allocated on the first call, for RS_VOTE_SWEEP_MAX thresholds
  double* sweep_wscore = nullptr;               // device: wscore [max_batch][RS_VOTE_SWEEP_MAX][RS_EVAL_GT_CAP][K], then wfrac of the same shape
  int* sweep_pairs = nullptr;
  size_t sweep_cells = 0;
  int ensure_vote_sweep_buffers();
  // the polygon geometry of the vote (rs_engine_fetch_votes_poly_*, poly_overlap.h): allocated on the first call
  double* pvote_frac = nullptr;                 // device: [max_batch][D][RS_EVAL_GT_CAP]
  double* pvote_area = nullptr;                 // device: [max_batch][RS_EVAL_GT_CAP]
  int* pvote_flagged = nullptr;                 // device: [max_batch]
  long long poly_forward = -1;                  // forward_index at the last rs_engine_fetch_polygons_async, and its batch
  int poly_tiles = 0;
  int ensure_poly_vote_buffers();
  // band histograms (rs_engine_fetch_band_hist_*, band_hist.h): allocated on the first call
  uint32_t* band_hist_dev = nullptr;            // device: [max_batch * RS_EVAL_GT_CAP][tile_c][256]
  hipEvent_t ev_band_tiles = nullptr;           // recorded on the copy stream behind the histogram kernel, the one reader of tiles_dev there
  bool band_tiles_pending = false;              // a write into tiles_dev on `stream` must wait for ev_band_tiles first
  int ensure_band_buffers();
  int wait_band_tiles();                        // in front of every write into tiles_dev; enqueues nothing unless band_tiles_pending

  // the steps of a result fetch, in the order the fetch entries enqueue them (engine.hip)
  int ensure_crop_header();
  int ensure_polygon_buffers();
  int ensure_eval_buffers();
  int launch_eval_labels(const void* layout, hipStream_t s);         // layout: the MtLayout of what eval_pinned holds; upload + canvas rasteriser
  int launch_eval_pairs(int n, hipStream_t s);                       // the pair counts of the last forward's masks against those canvases
  int launch_eval_counts(int n, const void* layout, hipStream_t s);  // both, in this order
  int begin_fetch(hipStream_t* s);                       // creates the copy stream on first use; it waits for the work enqueued on `stream` so far
  int launch_crops(int n, hipStream_t s);
  int launch_polygons(int n, double rdp_epsilon, hipStream_t s);
  int enqueue_dets(const rs_dets* o, int n, hipStream_t s, bool want_masks);
  int enqueue_crop_table(rs_mask_crops* c, int n, hipStream_t s);
  int end_fetch(hipStream_t s, hipEvent_t header);       // saturation snapshot, ev_copied, then the header event of the crops / polygons (null = none)
  int enqueue_crop_bytes(rs_mask_crops* c, hipStream_t s);

  // the precision of the activations, as the launchers take it (PreprocParams::out_f32, RoiAlignParams::f32, MaskPredictParams::f32)
  int prec_code() const { return f32 ? 1 : (split ? 2 : 0); }
  int planes() const { return split ? 2 : 1; }        // fp16 planes per activation / weight
  size_t esize() const { return f32 ? 4 : 2; }        // bytes per element of one plane

  int alloc(void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    RS_HIP(hipMalloc(p, bytes));
    allocs.push_back(*p);
    RS_HIP(hipMemsetAsync(*p, 0, bytes, stream));
    return RS_OK;
  }
  // A zeroed device buffer of the given shape, entered in the tensor table (rs_engine_tensor); buffers nobody inspects take plain alloc
  template <class T>
  int new_tensor(T** p, const std::string& name, int dtype, std::vector<int64_t> dims, int halo = 0) {
    TensorInfo t;
    t.name = name; t.dtype = dtype; t.ndim = (int)dims.size(); t.halo = halo;
    size_t nb = dt_size(dtype);
    for (size_t i = 0; i < dims.size(); ++i) { t.dims[i] = dims[i]; nb *= (size_t)dims[i]; }
    t.bytes = dtype == DT_SPLIT16 ? 2 * nb : nb;
    int rc = alloc((void**)p, t.bytes);
    if (rc) return rc;
    t.p = *p;
    tensors.push_back(t);
    return RS_OK;
  }
  int new_act(Act* a, const std::string& name, int N, int H, int W, int C, int pad) {
    a->N = N; a->H = H; a->W = W; a->C = C; a->pad = pad;
    a->lo = split ? (long long)N * a->Hp() * a->Wp() * C : 0;
    return new_tensor(&a->p, name, f32 ? DT_F32 : (split ? DT_SPLIT16 : DT_F16), {N, a->Hp(), a->Wp(), C}, pad);
  }
  // Appends a stage and returns it for its `fn`.  A stage that counts saturated values passes the address of its launch parameters'
  // `sat` field and gets the counter of its own position in `stages` (null in a trainer's forward engine).  Call it in a statement of
  // its own, before the lambda that copies the parameters: in `add_stage(..).fn = [p]..` the right-hand side is evaluated first.
  Stage& add_stage(const std::string& name, double flops_per_image, double bytes_per_image, unsigned long long** sat = nullptr) {
    if (sat) *sat = sat_dev ? sat_dev + stages.size() : nullptr;
    stages.emplace_back();
    Stage& st = stages.back();
    st.name = name; st.flops_per_image = flops_per_image; st.bytes_per_image = bytes_per_image;
    return st;
  }
  const BlobEntry* find(const std::string& n) {
    auto it = blob.find(n);
    return it == blob.end() ? nullptr : &it->second;
  }
  // GEMM weights of a layer: "<layer>.w" (fp16) or "<layer>.w32" in the fp32 validation mode
  // split-operand mode: "<layer>.ws" = fp16 [2][rows][Kpad] (hi rows, then lo rows, of the row-scaled weight) + "<layer>.wsi" fp32 [rows] (inverse scales)
  const BlobEntry* findw(const std::string& layer) { return find(layer + (f32 ? ".w32" : (split ? ".ws" : ".w"))); }
  int wrows(const BlobEntry* w) const { return (int)(split ? w->dims[0] / 2 : w->dims[0]); }
  // fills the split-operand fields of a conv whose weight entry is w (no-op in the other modes)
  int set_split(ConvParams* p, const std::string& wname, const BlobEntry* w, const Act* in, const Act* out, const Act* res, const Act* up, const Act* in2) {
    if (!split) return RS_OK;
    const BlobEntry* si = find(wname + ".wsi");
    RS_CHECK(si && si->dtype == DT_F32 && si->dims[0] >= w->dims[0] / 2 && (w->dims[0] & 1) == 0, RS_ERR_BLOB, "row scales of %s missing from blob (split-operand mode)", wname.c_str());
    p->split = 1;
    p->wscale = (const float*)si->dev;
    p->w_lo = (long long)(w->dims[0] / 2) * w->dims[1];
    if (in) p->in_lo = in->lo;
    if (out) p->out_lo = out->lo;
    if (res) p->res_lo = res->lo;
    if (up) p->up_lo = up->lo;
    if (in2) p->in2_lo = in2->lo;
    return RS_OK;
  }
  int parse_blob(const void* data, size_t nbytes);
  struct DeferredConv { ConvParams p; int m_per_image = 0; double flops = 0, bytes = 0; };
  struct ConvDesc {                  // one conv / linear stage (add_conv): ConvDesc{k, stride, pad, relu}, the rest by name
    int k = 1, stride = 1, pad = 0;
    bool relu = false;
    const Act* res = nullptr;        // residual added before the ReLU
    const Act* up = nullptr;         // coarser map added 2x-upsampled (FPN top-down path)
    int cin_real = 0;                // input channels in the FLOP count (stem: 3 of 8 padded channels); 0 = in.C
    int units_per_tile = 1;          // images of the conv per input tile (1 for feature maps, D for per-RoI maps)
    const int* m_count = nullptr;    // device-side count of units actually present
    const Act* in2 = nullptr;        // second K source: 1x1 taps at stride2 (projection shortcut folded into conv3)
    int stride2 = 1;
    DeferredConv* defer = nullptr;   // filled instead of a stage: the caller merges it into a multi-map launch (add_merged_convs)
  };
  int add_conv(const std::string& name, const std::string& wname, const Act& in, const Act& out, const ConvDesc& d);
  // ---- forward product on split operands (rs_trainer_set_fwd_mode): only the forward engine of an fp32 trainer carries it
  // (fwd_split_capable); every other engine launches exactly as before.  A conv / linear stage's launch comes from conv_stage_fn, which
  // reads fwd_mode when the stage runs: mode 1 on a shape conv_fwd_split_serves accepts = plane passes on X into fws_scratch, then the split
  // kernel on the layer's weight planes; else launch_conv(p, s, variant, glds).  The stages follow one another on one stream, so one
  // scratch serves them all.
  struct FwdSplitLayer {
    const float* w = nullptr;        // the folded fp32 forward weight [rows][kpad] (the blob's device copy; a trainer's fold rewrites it)
    int rows = 0, kpad = 0;
    half_t* planes = nullptr;        // [2 * rows][kpad], allocated at switch-on
    float* inv = nullptr;            // inverse row scales [rows]
  };
  bool fwd_split_capable = false;
  int fwd_mode = 0;
  std::vector<FwdSplitLayer> fws_layers;   // one per distinct weight matrix (the RPN's shared conv is one layer under five stages)
  void* fws_scratch = nullptr;
  long long fws_cap = 0;                   // elements of the largest X of any served stage at max_batch
  SplitRowsDesc* fws_table = nullptr;      // device: [all layers | the layers a fold rewrites]
  int fws_n_all = 0, fws_n_fold = 0;
  unsigned fws_rows_all = 0, fws_rows_fold = 0;
  std::function<int(int, hipStream_t)> conv_stage_fn(const ConvParams& p, int m_per_image, int variant, int glds);
  int fwd_split_enable(const std::set<const void*>& folded);   // first switch-on: scratch, planes, tables (`folded`: weights a fold rewrites)
  int fwd_split_weights(bool folded_only);                     // one table launch on `stream`
  int set_fwd_mode(int mode, const std::set<const void*>& folded);
  int add_merged_convs(const std::string& name, const std::vector<DeferredConv>& d);
  // ---- the graph builder: build() runs the sections below in order; `Graph` is what one section hands to the next
  // (the detections a forward returns are the det_* members above)
  struct Graph {
    Act x0, c1, res_out[4], P[5];
    Act rpn_t[RS_MAX_LEVELS];          // 3x3 RPN conv outputs (written only where the heads are not fused into it)
    float* rpn_ho[RS_MAX_LEVELS];      // RPN head outputs (objectness + deltas)
    float* prop_boxes = nullptr;
    int *prop_count = nullptr, *prop_level = nullptr, *prop_order = nullptr;
    float* pred = nullptr;             // box predictor output
    int *slot_list = nullptr, *det_total = nullptr;   // compacted detection slots of the batch, for the mask head
  };
  struct ResCursor {                   // running state of the residual stages, block to block
    Act cur;
    Act t1_pre;                        // conv1 output of the NEXT block when the previous block's fused tail already produced it
    bool have_t1 = false;
    int bott = 64, cout = 0;
  };
  int build();
  int build_input(Graph& g);
  int build_stem(Graph& g);
  int build_res_stages(Graph& g);
  int build_bottleneck(ResCursor& r, int si, int bi);
  int add_fused_tail(const std::string& nm, const std::string& next, const Act& t1, const Act& x, const Act& out, const Act* t1n, bool proj);
  int build_fpn(Graph& g);
  int build_rpn(Graph& g);
  int build_box_head(Graph& g);
  int build_mask_head(Graph& g);
  // FPN output convs / RPN 3x3 of all levels as one multi-map launch each
  bool merge_maps() const { return merge_levels && !f32 && rs_debug().conv_deep && use_glds > 0; }
  int add_nms_rule(const char* head, NmsParams* np, int group);
  RoiAlignParams roi_align_levels(const Graph& g) const;
  int run(const uint8_t* tiles, int n, int phase = -1);
  int run_stages(int n, bool record, int phase = -1, bool all_wide = false);
  int assign_phases();
  int use_graph = 0;
  int fuse_shortcut = 1;
  int fuse_bneck = 1;
  int fuse_stem = 1;      // stem conv + ReLU + max-pool as one launch (inference engines, fp16 path)
  bool frozen_fusions_only = false;   // a trainer's forward engine: layer fusions only where nothing is differentiated (stem + res2 at FREEZE_AT 2)
  int freeze_at = 2;                  // ... and its MODEL.BACKBONE.FREEZE_AT: below 2 res2 is built unfused, at 0 the stem too (inference engines: 2)
  int merge_levels = 1;   // FPN output convs / RPN 3x3 of all levels as one multi-map launch each (inference engines, fp16 path)
  long long forward_index = 0;
  // Saturation counts: one u64 per stage, indexed like `stages`; inference engines only (a trainer's forward engine: null).
  // Every forward zeroes the live array at its start and copies it to the snapshot at the end of its last phase; the fetches copy the
  // snapshot only, so a next forward that is already counting never races a result copy.
  static constexpr int kSatCap = 512;
  unsigned long long* sat_dev = nullptr;     // live counters of the forward in flight
  unsigned long long* sat_snap = nullptr;    // the last finished forward's
  unsigned long long* h_sat_copy = nullptr;  // pinned target of the fetch copies
  bool sat_copy_pending = false;
  std::vector<int64_t> h_sat;                // the most recent fetched forward's
  int sat_copy(hipStream_t s) {
    if (!sat_dev) return RS_OK;
    RS_HIP(hipMemcpyAsync(h_sat_copy, sat_snap, stages.size() * 8, hipMemcpyDeviceToHost, s));
    sat_copy_pending = true;
    return RS_OK;
  }
  void sat_publish() {
    if (!sat_copy_pending) return;
    h_sat.assign(h_sat_copy, h_sat_copy + stages.size());
    sat_copy_pending = false;
  }
  std::set<int> warmed;
  std::map<int, hipGraphExec_t> graphs;
};

// rs_engine_create, or with `for_trainer` the forward engine of an rs_trainer (rs_engine::frozen_fusions_only, ::freeze_at)
int engine_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int max_batch,
                  int tile_h, int tile_w, int tile_c, void* stream, bool for_trainer, rs_engine** out, int freeze_at = 2);
