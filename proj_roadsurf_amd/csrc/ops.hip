// librs_engine.so host side: the stand-alone operators rs_op_* of include/rs_engine.h -- one kernel launcher each on caller-owned device
// buffers, for the operator tests and the tools.  Nothing here touches an engine.
#include <string.h>

#include <vector>

#include "../../include/rs_engine.h"
#include "detect.h"
#include "polygon_pool.h"
#include "train.h"
#include "train_stats.h"
#include "val_ap.h"
#include "poly_vote.h"

namespace {

// Device scratch that lives for one operator call (the engine and the trainer own theirs for good).  Leaving the scope waits for the
// stream the launch went to, if anything was allocated, and frees it -- on the error returns too.
struct OpScratch {
  hipStream_t stream;
  void* held[2] = {nullptr, nullptr};
  int n = 0;
  explicit OpScratch(void* s) : stream((hipStream_t)s) {}
  OpScratch(const OpScratch&) = delete;
  OpScratch& operator=(const OpScratch&) = delete;
  int alloc(void** p, size_t bytes) {
    RS_CHECK(n < 2, RS_ERR_ARG, "OpScratch: more than two buffers");
    RS_HIP(hipMalloc(p, bytes));
    held[n++] = *p;
    return RS_OK;
  }
  hipError_t sync() const { return n ? hipStreamSynchronize(stream) : hipSuccess; }
  ~OpScratch() {
    (void)sync();
    for (int i = 0; i < n; ++i) (void)hipFree(held[i]);
  }
};

}  // namespace

// ---- rs_solver: the checks rs_trainer_set_solver, rs_op_sgd_segments and rs_host_sgd_segments share, and the values of one launch
int sgd_solver_check(const char* who, const rs_solver* sv) {
  RS_CHECK(sv, RS_ERR_ARG, "%s: null solver", who);
  RS_CHECK(sv->struct_size == (int32_t)sizeof(rs_solver), RS_ERR_ARG, "%s: rs_solver.struct_size %d, expected %d", who, sv->struct_size, (int)sizeof(rs_solver));
  RS_CHECK(sv->nesterov == 0 || sv->nesterov == 1, RS_ERR_ARG, "%s: nesterov %d (0 / 1)", who, sv->nesterov);
  RS_CHECK(sv->bias_lr_factor >= 0.f && sv->bias_lr_factor < INFINITY, RS_ERR_ARG, "%s: bias_lr_factor %g", who, (double)sv->bias_lr_factor);
  RS_CHECK(sv->has_weight_decay_bias == 0 || sv->has_weight_decay_bias == 1, RS_ERR_ARG, "%s: has_weight_decay_bias %d (0 / 1)", who, sv->has_weight_decay_bias);
  RS_CHECK(!sv->has_weight_decay_bias || (sv->weight_decay_bias >= 0.f && sv->weight_decay_bias < INFINITY), RS_ERR_ARG, "%s: weight_decay_bias %g", who,
           (double)sv->weight_decay_bias);
  RS_CHECK(sv->clip_type >= SGD_CLIP_NONE && sv->clip_type <= SGD_CLIP_FULL_MODEL, RS_ERR_ARG, "%s: clip_type %d (0 none, 1 value, 2 norm, 3 full_model)", who, sv->clip_type);
  RS_CHECK(sv->clip_type == SGD_CLIP_NONE || (sv->clip_value > 0.f && sv->clip_value < INFINITY), RS_ERR_ARG, "%s: clip_value %g (must be > 0)", who, (double)sv->clip_value);
  RS_CHECK(sv->clip_type < SGD_CLIP_NORM || sv->norm_type == 2.0f || sv->norm_type == INFINITY, RS_ERR_ARG, "%s: norm_type %g (2 or inf)", who, (double)sv->norm_type);
  return RS_OK;
}
int sgd_solver_hyper(const char* who, const rs_solver& sv, float lr, float momentum, float weight_decay, float inv_scale, SgdHyper* h, int* norm_inf) {
  RS_CHECK(!sv.nesterov || momentum > 0.f, RS_ERR_ARG, "%s: Nesterov momentum needs momentum > 0, got %g", who, (double)momentum);
  h->lr = lr; h->lr_bias = lr * sv.bias_lr_factor;
  h->wd = weight_decay; h->wd_bias = sv.has_weight_decay_bias ? sv.weight_decay_bias : weight_decay;
  h->momentum = momentum; h->inv_scale = inv_scale;
  h->clip_value = sv.clip_type == SGD_CLIP_NONE ? 0.f : sv.clip_value;
  h->nesterov = sv.nesterov; h->clip_type = sv.clip_type;
  *norm_inf = sv.clip_type >= SGD_CLIP_NORM && sv.norm_type == INFINITY;
  return RS_OK;
}

extern "C" {

// rs_fdiv (common.h) as an operator, for its test: out[i] = a[i] / b[i] through the device code's division
__global__ void fdiv_kernel(const float* a, const float* b, float* out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = rs_fdiv(a[i], b[i]);
}
int rs_op_fdiv(const float* a, const float* b, float* out, int64_t n, void* stream) {
  RS_CHECK(a && b && out && n > 0, RS_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(fdiv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, out, (long long)n);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int rs_memcpy_d2h(void* dst, const void* src, size_t n) {
  RS_HIP(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
  return RS_OK;
}
int rs_memcpy_h2d(void* dst, const void* src, size_t n) {
  RS_HIP(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
  return RS_OK;
}

int rs_op_conv_variant(int m, int cin, int k, int cout, int cin2, int deconv2x, int out_f32, int* stages_out) {
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.M = m; p.Cin = cin; p.KH = p.KW = k; p.Cout = cout; p.mode = deconv2x ? 1 : 0; p.out_f32 = out_f32;
  p.stride = 1; p.in_Cs = cin; p.out_Cs = cout;
  p.Kpad = (k * k * (cin < 64 ? 8 : cin) + cin2 + 63) / 64 * 64;
  if (cin < 64 && k == 7) p.Kpad = 256;       // the stem's padded tap rows (weights.py STEM_KW_PAD)
  static const half_t dummy = (half_t)0;
  if (cin2 > 0) { p.in2 = &dummy; p.Cin2 = cin2; }
  const int v = conv_choose_variant(p, -1, 1);
  if (stages_out) *stages_out = p.stages;
  return cin < 64 ? 5 : v;
}

// The same rule for the split-operand mode (ConvParams::split), with the stride and the fused mask predictor (deconv 2x2 s2 + predictor: 4 * cout rows) it depends on
int rs_op_conv_variant_split(int m, int cin, int k, int stride, int cout, int cin2, int deconv_predict, int* stages_out) {
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.M = m; p.Cin = cin; p.KH = p.KW = k; p.Cout = cout; p.mode = deconv_predict ? 2 : 0;
  p.stride = stride; p.in_Cs = cin; p.out_Cs = cout; p.split = 1;
  p.Kpad = (k * k * (cin < 64 ? 8 : cin) + cin2 + 63) / 64 * 64;
  if (cin < 64 && k == 7) p.Kpad = 256;
  static const half_t dummy = (half_t)0;
  if (cin2 > 0) { p.in2 = &dummy; p.Cin2 = cin2; }
  const int v = conv_choose_variant(p, -1, 1);
  if (stages_out) *stages_out = p.stages;
  return cin < 64 ? 5 : v;
}

static long long* g_conv_probe = nullptr;   // -DRS_CLOCK_PROBE diagnostic builds: see rs_debug_set_conv_probe
static thread_local unsigned long long* g_op_sat = nullptr;   // rs_op_set_saturation_counter
struct SplitArgs { long long in_lo, w_lo, out_lo, res_lo, up_lo; const float* wscale; };
static int op_conv2d(const void* in, const void* w, const float* bias, void* out, const void* residual, const void* upsample_add,
                     int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad,
                     int out_halo, int relu, int out_f32, int deconv2x, int variant, int use_glds, void* stream,
                     const void* in2, int h2, int w2, int cin2, int in2_halo, int stride2, const SplitArgs* sa = nullptr) {
  RS_CHECK(in && w && bias && out, RS_ERR_ARG, "null argument");
  RS_CHECK(in_halo >= pad, RS_ERR_ARG, "input halo %d < pad %d", in_halo, pad);
  const int ho = (hi + 2 * pad - kh) / stride + 1, wo = (wi + 2 * pad - kw) / stride + 1;
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.in = (const half_t*)in; p.w = (const half_t*)w; p.bias = bias; p.out = out;
  p.res = (const half_t*)residual; p.up = (const half_t*)upsample_add;
  p.M = n * ho * wo; p.Ho = ho; p.Wo = wo;
  p.in_Hp = hi + 2 * in_halo; p.in_Wp = wi + 2 * in_halo; p.in_Cs = cin; p.in_off = in_halo - pad;
  p.stride = stride; p.KH = kh; p.KW = kw; p.Cin = cin; p.Kpad = kpad; p.Cout = cout;
  const int oh = deconv2x ? 2 * ho : ho, ow = deconv2x ? 2 * wo : wo;
  p.out_Hp = oh + 2 * out_halo; p.out_Wp = ow + 2 * out_halo; p.out_Cs = cout; p.out_pad = out_halo;
  if (upsample_add) { p.up_Hp = ho / 2 + 2 * out_halo; p.up_Wp = wo / 2 + 2 * out_halo; p.up_Cs = cout; p.up_pad = out_halo; }
  p.relu = relu; p.mode = deconv2x ? 1 : 0; p.out_f32 = out_f32;
  p.probe = g_conv_probe;
  p.sat = g_op_sat;
  if (sa) {
    RS_CHECK(sa->wscale && !in2, RS_ERR_ARG, "split-operand conv: row scales missing (or a second K source, which the operator does not take)");
    p.split = 1; p.in_lo = sa->in_lo; p.w_lo = sa->w_lo; p.out_lo = sa->out_lo; p.res_lo = sa->res_lo; p.up_lo = sa->up_lo; p.wscale = sa->wscale;
  }
  if (in2) {
    RS_CHECK(stride2 >= 1 && (ho - 1) * stride2 < h2 && (wo - 1) * stride2 < w2, RS_ERR_ARG, "second source geometry");
    p.in2 = (const half_t*)in2; p.in2_Hp = h2 + 2 * in2_halo; p.in2_Wp = w2 + 2 * in2_halo; p.in2_Cs = cin2;
    p.in2_off = in2_halo; p.stride2 = stride2; p.Cin2 = cin2;
  }
  OpScratch scratch(stream);
  if (cin < 64 && use_glds >= 0) {
    RS_CHECK(cin == 8, RS_ERR_UNSUPPORTED, "small-Cin path needs cin == 8");
    std::vector<int> koff(kpad / 8, 0);
    for (int t = 0; t < kh * kw && t < (int)koff.size(); ++t) koff[t] = ((t / kw) * p.in_Wp + (t % kw)) * cin;
    int* koff_dev = nullptr;
    { int rc = scratch.alloc((void**)&koff_dev, koff.size() * 4); if (rc) return rc; }
    RS_HIP(hipMemcpy(koff_dev, koff.data(), koff.size() * 4, hipMemcpyHostToDevice));
    p.koff = koff_dev;
  }
  return launch_conv(p, (hipStream_t)stream, variant, use_glds);
}

int rs_debug_set_conv_probe(void* buffer) { g_conv_probe = (long long*)buffer; return RS_OK; }
int rs_op_set_saturation_counter(void* dev_u64) { g_op_sat = (unsigned long long*)dev_u64; return RS_OK; }

int rs_op_conv2d(const void* in, const void* w, const float* bias, void* out, const void* residual, const void* upsample_add,
                 int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad,
                 int out_halo, int relu, int out_f32, int deconv2x, int variant, int use_glds, void* stream) {
  return op_conv2d(in, w, bias, out, residual, upsample_add, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, out_halo,
                   relu, out_f32, deconv2x, variant, use_glds, stream, nullptr, 0, 0, 0, 0, 1);
}

// The same convolution in the split-operand precision mode (rs_spec.precision == 2): every fp16 tensor is a hi plane with its lo plane `*_lo`
// ELEMENTS behind it (value = hi + lo), the weight rows are scaled by a power of two per row and `wscale` holds the inverses.
int rs_op_conv2d_split(const void* in, int64_t in_lo, const void* w, int64_t w_lo, const float* wscale, const float* bias, void* out, int64_t out_lo,
                       const void* residual, int64_t res_lo, const void* upsample_add, int64_t up_lo,
                       int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad,
                       int out_halo, int relu, int out_f32, int deconv2x, int variant, void* stream) {
  SplitArgs sa = {in_lo, w_lo, out_lo, res_lo, up_lo, wscale};
  return op_conv2d(in, w, bias, out, residual, upsample_add, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, out_halo,
                   relu, out_f32, deconv2x, variant, 1, stream, nullptr, 0, 0, 0, 0, 1, &sa);
}

// The mask head's fused deconv 2x2 s2 + ReLU + predictor (ConvParams::mode 2) in the split-operand mode on caller tensors: `in` [entries][side + 2][side + 2][256]
// (halo 1) as hi / lo planes, w [4 * 256][256] scaled rows (+ lo plane), bias / wscale [1024], dot_w [classes][256] fp32, slot[entry] -> row of `logits`
// [slots][2 side][2 side] (bias-free logits), cls[slot] the class.  Rows = min(entries, *count_dev) * side^2.  Variants 14 / 10 / 0 accumulate into `logits` (the
// caller zeroes it), 28 - 31 store.
int rs_op_deconv_predict_split(const void* in, int64_t in_lo, const void* w, int64_t w_lo, const float* wscale, const float* bias, const float* dot_w, int classes,
                               const int32_t* cls, const int32_t* slot, const int32_t* count_dev, float* logits, int entries, int side, int variant, void* stream) {
  RS_CHECK(in && w && wscale && bias && dot_w && cls && slot && logits && entries > 0 && side > 0 && classes > 0, RS_ERR_ARG, "deconv_predict_split: bad argument");
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.in = (const half_t*)in; p.w = (const half_t*)w; p.bias = bias; p.wscale = wscale;
  p.split = 1; p.in_lo = in_lo; p.w_lo = w_lo;
  p.M = entries * side * side; p.Ho = side; p.Wo = side;
  p.in_Hp = side + 2; p.in_Wp = side + 2; p.in_Cs = 256; p.in_off = 1; p.stride = 1; p.KH = p.KW = 1; p.Cin = 256; p.Kpad = 256; p.Cout = 256;
  p.out_Hp = 2 * side; p.out_Wp = 2 * side; p.out_Cs = 256; p.relu = 1; p.mode = 2;
  p.m_count = count_dev; p.m_mul = side * side;
  p.dot_w = dot_w; p.dot_cls = cls; p.dot_slot = slot; p.dot_out = logits; p.dot_k = classes;
  return launch_conv(p, (hipStream_t)stream, variant, 1);
}

int rs_op_conv2d_dual(const void* in, const void* in2, const void* w, const float* bias, void* out,
                      int n, int hi, int wi, int cin, int in_halo, int kh, int kw, int stride, int pad,
                      int h2, int w2, int cin2, int in2_halo, int stride2,
                      int cout, int kpad, int out_halo, int relu, int variant, void* stream) {
  RS_CHECK(in2, RS_ERR_ARG, "null argument");
  return op_conv2d(in, w, bias, out, nullptr, nullptr, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, out_halo,
                   relu, 0, 0, variant, 1, stream, in2, h2, w2, cin2, in2_halo, stride2);
}

int rs_op_bneck_tail(const void* t1, const void* w2, const float* b2, const void* w3p, const float* b3, const void* x, void* out,
                     const void* w1p, const float* b1, void* t1n, const void* x0, const void* wsc, int n, int h, int w, int width, void* stream) {
  RS_CHECK(t1 && w2 && b2 && w3p && b3 && out && n > 0 && h > 0 && w > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(width == 64 || width == 128, RS_ERR_UNSUPPORTED, "bneck_tail: bottleneck width %d (64 or 128)", width);
  BneckParams p;
  memset(&p, 0, sizeof p);
  p.t1 = (const half_t*)t1; p.w2 = (const half_t*)w2; p.b2 = b2; p.w3p = (const half_t*)w3p; p.b3 = b3; p.x = (const half_t*)x; p.out = (half_t*)out;
  p.w1p = (const half_t*)w1p; p.b1 = b1; p.t1n = (half_t*)t1n; p.x0 = (const half_t*)x0; p.wsc = (const half_t*)wsc;
  p.M = n * h * w; p.H = h; p.W = w; p.Hp = h + 2; p.Wp = w + 2; p.CB = width / 64;
  p.sat = g_op_sat;
  return launch_bneck_tail(p, (hipStream_t)stream);
}

int rs_op_bneck_tail_split(const void* t1, int64_t t1_lo, const void* w2, const float* s2, const float* b2, const void* w3p, const float* s3, const float* b3,
                           const void* x, int64_t x_lo, void* out, int64_t out_lo, const void* w1p, const float* s1, const float* b1, void* t1n, int64_t t1n_lo,
                           const void* x0, int64_t x0_lo, int n, int h, int w, int width, void* stream) {
  RS_CHECK(t1 && w2 && s2 && b2 && w3p && s3 && b3 && (x || x0) && out && n > 0 && h > 0 && w > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(width == 64 || width == 128, RS_ERR_UNSUPPORTED, "bneck_tail_split: bottleneck width %d (64 or 128)", width);
  BneckSplitParams p;
  memset(&p, 0, sizeof p);
  p.t1 = (const half_t*)t1; p.t1_lo = t1_lo;
  p.w2 = (const half_t*)w2; p.w2_lo = (long long)width * 9 * width; p.s2 = s2; p.b2 = b2;
  p.w3p = (const half_t*)w3p; p.w3_lo = 4ll * width * (width + (x0 ? 64 : 0)); p.s3 = s3; p.b3 = b3;
  p.x = (const half_t*)x; p.x_lo = x_lo; p.x0 = (const half_t*)x0; p.x0_lo = x0_lo; p.out = (half_t*)out; p.out_lo = out_lo;
  p.w1p = (const half_t*)w1p; p.w1_lo = 4ll * width * width; p.s1 = s1; p.b1 = b1; p.t1n = (half_t*)t1n; p.t1n_lo = t1n_lo;
  p.M = n * h * w; p.H = h; p.W = w; p.Hp = h + 2; p.Wp = w + 2; p.CB = width / 64;
  p.sat = g_op_sat;
  return launch_bneck_tail_split(p, (hipStream_t)stream);
}

int rs_op_mask_overlap(const uint8_t* det_masks, int n_det, const uint8_t* label_masks, int n_labels, int h, int w, int32_t* inter,
                       int32_t* label_area, void* stream) {
  return launch_mask_overlap(det_masks, n_det, label_masks, n_labels, h, w, inter, label_area, (hipStream_t)stream);
}


// canvas_raster_kernel as an operator, the counterpart of rs_op_mask_targets: host pointers in, packs and uploads the polygons,
// rasterises one canvas per instance and copies the bit-packed masks back.  Arguments are refused before a device is touched.
int rs_op_rasterize_canvas(const double* polys, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, int n_inst,
                           int side, uint8_t* out) {
  RS_CHECK(inst_first && n_inst >= 0 && (out || n_inst == 0), RS_ERR_ARG, "rasterize_canvas: null table");
  RS_CHECK(side >= 1 && side <= CR_MAX_SIDE, RS_ERR_ARG, "rasterize_canvas: side %d outside [1, %d]", side, CR_MAX_SIDE);
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, n_inst, 0, &L); if (rc) return rc; }
  RS_CHECK(L.n_doubles <= (size_t)MT_MAX_DOUBLES, RS_ERR_UNSUPPORTED, "rasterize_canvas: more than %d doubles of polygons", MT_MAX_DOUBLES);
  if (n_inst == 0) return RS_OK;
  std::vector<uint8_t> host(L.bytes);
  const int32_t zero = 0;
  mt_pack(host.data(), L, polys, poly_off, poly_len, inst_first, &zero);
  const size_t bytes = (size_t)n_inst * side * ((side + 7) / 8);
  OpScratch scratch(nullptr);
  uint8_t *pool = nullptr, *m = nullptr;
  { int rc = scratch.alloc((void**)&pool, L.bytes); if (rc) return rc; }
  { int rc = scratch.alloc((void**)&m, bytes); if (rc) return rc; }
  RS_HIP(hipMemcpy(pool, host.data(), L.bytes, hipMemcpyHostToDevice));
  CanvasRasterParams q;
  memset(&q, 0, sizeof q);
  q.inst_first = (const int*)(pool + L.o_inst); q.poly_off = (const int*)(pool + L.o_off); q.poly_len = (const int*)(pool + L.o_len);
  q.polys = (const double*)(pool + L.o_xy); q.out = m; q.n_inst = n_inst; q.side = side;
  { int rc = launch_canvas_raster(q, nullptr); if (rc) return rc; }
  RS_HIP(hipMemcpy(out, m, bytes, hipMemcpyDeviceToHost));
  return RS_OK;
}

// mask_pair_counts_kernel on caller-owned device memory (see include/rs_engine.h)
int rs_op_mask_pair_counts(const uint8_t* det_masks, const int32_t* det_count, int n_tiles, int slots, const uint8_t* gt_masks,
                           const int32_t* tile_first, int gt_cap, int side, int32_t* inter, int32_t* det_area, int32_t* gt_area, void* stream) {
  RS_CHECK(det_masks && det_count && tile_first && inter && det_area && gt_area, RS_ERR_ARG, "mask_pair_counts: null buffer");
  RS_CHECK(side >= 1 && side <= CR_MAX_SIDE, RS_ERR_ARG, "mask_pair_counts: side %d outside [1, %d]", side, CR_MAX_SIDE);
  RS_CHECK(n_tiles >= 1 && slots >= 1 && gt_cap >= 1, RS_ERR_ARG, "mask_pair_counts: %d tiles, %d slots, %d ground truths per tile", n_tiles, slots, gt_cap);
  PairCountParams q;
  memset(&q, 0, sizeof q);
  q.det_masks = det_masks; q.det_count = det_count; q.gt_masks = gt_masks; q.tile_first = tile_first;
  q.inter = inter; q.det_area = det_area; q.gt_area = gt_area; q.n = n_tiles; q.D = slots; q.g_cap = gt_cap;
  q.bytes = (long long)side * ((side + 7) / 8);
  return launch_mask_pair_counts(q, (hipStream_t)stream);
}

// COCOeval's evaluateImg on caller-owned tables (see include/rs_engine.h): device pointers enqueued on `stream`, or host pointers
static_assert(CM_MAX_CLASSES == RS_MAX_CLASSES && CM_MAX_GT == RS_EVAL_GT_CAP, "coco_match.h restates the header's capacities");
static int coco_match_params(const char* who, CocoMatchParams* q, const float* det_boxes, const float* det_scores, const int32_t* det_classes,
                             const int32_t* det_count, const double* gt_boxes, const int32_t* gt_classes, const int32_t* tile_first,
                             const int32_t* inter, const int32_t* det_area, const int32_t* gt_area, const double* iou_thrs, int n_tiles,
                             int num_classes, int slots, int gt_cap, int32_t* order, int32_t* class_first, int32_t* gt_per_class,
                             uint32_t* matched, uint32_t* ignored, int32_t* npig) {
  RS_CHECK(iou_thrs, RS_ERR_ARG, "%s: null table (the IoU thresholds)", who);
  memset(q, 0, sizeof *q);
  q->det_boxes = det_boxes; q->det_scores = det_scores; q->det_classes = det_classes; q->det_count = det_count;
  q->gt_boxes = gt_boxes; q->gt_classes = gt_classes; q->tile_first = tile_first; q->inter = inter; q->det_area = det_area; q->gt_area = gt_area;
  q->order = order; q->class_first = class_first; q->gt_per_class = gt_per_class; q->matched = matched; q->ignored = ignored; q->npig = npig;
  for (int i = 0; i < CM_THRS; ++i) q->thrs[i] = iou_thrs[i];
  q->n = n_tiles; q->K = num_classes; q->D = slots; q->g_cap = gt_cap;
  return coco_match_check(who, *q);
}
int rs_op_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes, const int32_t* det_count,
                     const double* gt_boxes, const int32_t* gt_classes, const int32_t* tile_first, const int32_t* inter,
                     const int32_t* det_area, const int32_t* gt_area, const double* iou_thrs, int n_tiles, int num_classes, int slots,
                     int gt_cap, int32_t* order, int32_t* class_first, int32_t* gt_per_class, uint32_t* matched, uint32_t* ignored,
                     int32_t* npig, void* stream) {
  CocoMatchParams q;
  { int rc = coco_match_params("rs_op_coco_match", &q, det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_classes, tile_first, inter, det_area,
                               gt_area, iou_thrs, n_tiles, num_classes, slots, gt_cap, order, class_first, gt_per_class, matched, ignored, npig);
    if (rc) return rc; }
  return launch_coco_match(q, (hipStream_t)stream);
}
int rs_host_coco_match(const float* det_boxes, const float* det_scores, const int32_t* det_classes, const int32_t* det_count,
                       const double* gt_boxes, const int32_t* gt_classes, const int32_t* tile_first, const int32_t* inter,
                       const int32_t* det_area, const int32_t* gt_area, const double* iou_thrs, int n_tiles, int num_classes, int slots,
                       int gt_cap, int32_t* order, int32_t* class_first, int32_t* gt_per_class, uint32_t* matched, uint32_t* ignored,
                       int32_t* npig) {
  CocoMatchParams q;
  { int rc = coco_match_params("rs_host_coco_match", &q, det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_classes, tile_first, inter, det_area,
                               gt_area, iou_thrs, n_tiles, num_classes, slots, gt_cap, order, class_first, gt_per_class, matched, ignored, npig);
    if (rc) return rc; }
  return host_coco_match(q);          // val_ap.hip: the float64 arithmetic is compiled there, without mul+add contraction
}

// The road cover vote on caller-owned tables (see include/rs_engine.h): device pointers enqueued on `stream`, or host pointers
static_assert(RV_MAX_CLASSES == RS_MAX_CLASSES && RV_MAX_GT == RS_EVAL_GT_CAP && RV_MAX_SLOTS == CM_MAX_SLOTS, "road_vote.h restates the header's capacities");
static int road_vote_params(const char* who, RoadVoteParams* q, const float* det_scores, const int32_t* det_classes, const int32_t* det_count,
                            const int32_t* tile_first, const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots,
                            int gt_cap, double threshold, double* wscore, double* wfrac, int32_t* pairs) {
  memset(q, 0, sizeof *q);
  q->det_scores = det_scores; q->det_classes = det_classes; q->det_count = det_count; q->tile_first = tile_first; q->inter = inter;
  q->gt_area = gt_area; q->wscore = wscore; q->wfrac = wfrac; q->pairs = pairs; q->threshold = threshold;
  q->n = n_tiles; q->K = num_classes; q->D = slots; q->g_cap = gt_cap;
  return road_vote_check(who, *q);
}
int rs_op_road_votes(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                     const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap, double threshold,
                     double* wscore, double* wfrac, int32_t* pairs, void* stream) {
  RoadVoteParams q;
  { int rc = road_vote_params("rs_op_road_votes", &q, det_scores, det_classes, det_count, tile_first, inter, gt_area, n_tiles, num_classes, slots, gt_cap,
                              threshold, wscore, wfrac, pairs);
    if (rc) return rc; }
  return launch_road_votes(q, (hipStream_t)stream);
}
int rs_host_road_votes(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                       const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap, double threshold,
                       double* wscore, double* wfrac, int32_t* pairs) {
  RoadVoteParams q;
  { int rc = road_vote_params("rs_host_road_votes", &q, det_scores, det_classes, det_count, tile_first, inter, gt_area, n_tiles, num_classes, slots, gt_cap,
                              threshold, wscore, wfrac, pairs);
    if (rc) return rc; }
  return host_road_votes(q);          // val_ap.hip: the float64 arithmetic is compiled there, without mul+add contraction
}

// The vote for a list of thresholds (road_vote.h, THE SWEEP): `thresholds` is a host pointer in both entries, copied into the parameters
static_assert(RV_SWEEP_MAX == RS_VOTE_SWEEP_MAX, "road_vote.h restates the header's sweep capacity");
static int road_vote_sweep_params(const char* who, RoadVoteSweepParams* q, const float* det_scores, const int32_t* det_classes,
                                  const int32_t* det_count, const int32_t* tile_first, const int32_t* inter, const int32_t* gt_area, int n_tiles,
                                  int num_classes, int slots, int gt_cap, const double* thresholds, int n_thresholds, double* wscore,
                                  double* wfrac, int32_t* pairs) {
  memset(q, 0, sizeof *q);
  q->det_scores = det_scores; q->det_classes = det_classes; q->det_count = det_count; q->tile_first = tile_first; q->inter = inter;
  q->gt_area = gt_area; q->wscore = wscore; q->wfrac = wfrac; q->pairs = pairs;
  q->n = n_tiles; q->K = num_classes; q->D = slots; q->g_cap = gt_cap; q->T = n_thresholds;
  RS_CHECK(thresholds, RS_ERR_ARG, "%s: null threshold list", who);
  for (int j = 0; j < n_thresholds && j < RV_SWEEP_MAX; ++j) q->thresholds[j] = thresholds[j];
  return road_vote_sweep_check(who, *q);
}
int rs_op_road_votes_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                           const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap,
                           const double* thresholds, int n_thresholds, double* wscore, double* wfrac, int32_t* pairs, void* stream) {
  RoadVoteSweepParams q;
  { int rc = road_vote_sweep_params("rs_op_road_votes_sweep", &q, det_scores, det_classes, det_count, tile_first, inter, gt_area, n_tiles, num_classes,
                                    slots, gt_cap, thresholds, n_thresholds, wscore, wfrac, pairs);
    if (rc) return rc; }
  return launch_road_votes_sweep(q, (hipStream_t)stream);
}
int rs_host_road_votes_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                             const int32_t* inter, const int32_t* gt_area, int n_tiles, int num_classes, int slots, int gt_cap,
                             const double* thresholds, int n_thresholds, double* wscore, double* wfrac, int32_t* pairs) {
  RoadVoteSweepParams q;
  { int rc = road_vote_sweep_params("rs_host_road_votes_sweep", &q, det_scores, det_classes, det_count, tile_first, inter, gt_area, n_tiles,
                                    num_classes, slots, gt_cap, thresholds, n_thresholds, wscore, wfrac, pairs);
    if (rc) return rc; }
  return host_road_votes_sweep(q);    // val_ap.hip: the float64 arithmetic is compiled there, without mul+add contraction
}

// The polygon geometry of the vote (poly_overlap.h; see include/rs_engine.h): overlaps of the polygoniser's tables with the labels' rings,
// then the sweep on those weights.  Device pointers enqueued on `stream`, or host pointers.
static_assert(PO_HDR == RS_POLY_HDR, "poly_overlap.h restates the polygon header's width");
static int poly_overlap_params(const char* who, PolyOverlapParams* q, const int32_t* header, const int32_t* poly_ring_count, const int32_t* ring_len,
                               const int16_t* xy, const int32_t* det_count, const int32_t* tile_first, const int32_t* inst_first,
                               const int32_t* poly_off, const int32_t* poly_len, const double* polys, int n_tiles, int slots, int gt_cap,
                               int raw_areas, double* frac, double* label_area, int32_t* flagged) {
  memset(q, 0, sizeof *q);
  q->header = header; q->poly_ring_count = poly_ring_count; q->ring_len = ring_len; q->xy = xy; q->det_count = det_count;
  q->tile_first = tile_first; q->inst_first = inst_first; q->poly_off = poly_off; q->poly_len = poly_len; q->polys = polys;
  q->frac = frac; q->label_area = label_area; q->flagged = flagged;
  q->n = n_tiles; q->D = slots; q->g_cap = gt_cap; q->raw_areas = raw_areas;
  return poly_overlap_check(who, *q);
}
int rs_op_polygon_overlaps(const int32_t* header, const int32_t* poly_ring_count, const int32_t* ring_len, const int16_t* xy,
                           const int32_t* det_count, const int32_t* tile_first, const int32_t* inst_first, const int32_t* poly_off,
                           const int32_t* poly_len, const double* polys, int n_tiles, int slots, int gt_cap, int raw_areas, double* frac,
                           double* label_area, int32_t* flagged, void* stream) {
  PolyOverlapParams q;
  { int rc = poly_overlap_params("rs_op_polygon_overlaps", &q, header, poly_ring_count, ring_len, xy, det_count, tile_first, inst_first, poly_off, poly_len,
                                 polys, n_tiles, slots, gt_cap, raw_areas, frac, label_area, flagged);
    if (rc) return rc; }
  return launch_poly_overlaps(q, (hipStream_t)stream);
}
int rs_host_polygon_overlaps(const int32_t* header, const int32_t* poly_ring_count, const int32_t* ring_len, const int16_t* xy,
                             const int32_t* det_count, const int32_t* tile_first, const int32_t* inst_first, const int32_t* poly_off,
                             const int32_t* poly_len, const double* polys, int n_tiles, int slots, int gt_cap, int raw_areas, double* frac,
                             double* label_area, int32_t* flagged) {
  PolyOverlapParams q;
  { int rc = poly_overlap_params("rs_host_polygon_overlaps", &q, header, poly_ring_count, ring_len, xy, det_count, tile_first, inst_first, poly_off,
                                 poly_len, polys, n_tiles, slots, gt_cap, raw_areas, frac, label_area, flagged);
    if (rc) return rc; }
  return host_poly_overlaps(q);       // poly_vote.hip: the float64 arithmetic is compiled there, without mul+add contraction
}

static int road_vote_area_sweep_params(const char* who, RoadVoteAreaSweepParams* q, const float* det_scores, const int32_t* det_classes,
                                       const int32_t* det_count, const int32_t* tile_first, const double* frac, int n_tiles, int num_classes,
                                       int slots, int gt_cap, const double* thresholds, int n_thresholds, double* wscore, double* wfrac,
                                       int32_t* pairs) {
  memset(q, 0, sizeof *q);
  q->det_scores = det_scores; q->det_classes = det_classes; q->det_count = det_count; q->tile_first = tile_first; q->frac = frac;
  q->wscore = wscore; q->wfrac = wfrac; q->pairs = pairs;
  q->n = n_tiles; q->K = num_classes; q->D = slots; q->g_cap = gt_cap; q->T = n_thresholds;
  RS_CHECK(thresholds, RS_ERR_ARG, "%s: null threshold list", who);
  for (int j = 0; j < n_thresholds && j < RV_SWEEP_MAX; ++j) q->thresholds[j] = thresholds[j];
  return road_vote_area_sweep_check(who, *q);
}
int rs_op_road_votes_area_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                                const double* frac, int n_tiles, int num_classes, int slots, int gt_cap, const double* thresholds,
                                int n_thresholds, double* wscore, double* wfrac, int32_t* pairs, void* stream) {
  RoadVoteAreaSweepParams q;
  { int rc = road_vote_area_sweep_params("rs_op_road_votes_area_sweep", &q, det_scores, det_classes, det_count, tile_first, frac, n_tiles, num_classes,
                                         slots, gt_cap, thresholds, n_thresholds, wscore, wfrac, pairs);
    if (rc) return rc; }
  return launch_road_votes_area_sweep(q, (hipStream_t)stream);
}
int rs_host_road_votes_area_sweep(const float* det_scores, const int32_t* det_classes, const int32_t* det_count, const int32_t* tile_first,
                                  const double* frac, int n_tiles, int num_classes, int slots, int gt_cap, const double* thresholds,
                                  int n_thresholds, double* wscore, double* wfrac, int32_t* pairs) {
  RoadVoteAreaSweepParams q;
  { int rc = road_vote_area_sweep_params("rs_host_road_votes_area_sweep", &q, det_scores, det_classes, det_count, tile_first, frac, n_tiles,
                                         num_classes, slots, gt_cap, thresholds, n_thresholds, wscore, wfrac, pairs);
    if (rc) return rc; }
  return host_road_votes_area_sweep(q);
}

// The band histograms under label canvases on caller-owned tables (see include/rs_engine.h): device pointers enqueued on `stream`, or
// host pointers
static_assert(BH_MAX_SIDE == CR_MAX_SIDE, "band_hist.h restates the canvases' capacity");
static int band_hist_params(const char* who, BandHistParams* q, const uint8_t* tiles, const uint8_t* label_masks, const int32_t* tile_first,
                            int n_tiles, int n_inst, int side, int channels, uint32_t* hist) {
  memset(q, 0, sizeof *q);
  q->tiles = tiles; q->label_masks = label_masks; q->tile_first = tile_first; q->hist = hist;
  q->n = n_tiles; q->n_inst = n_inst; q->side = side; q->C = channels;
  return band_hist_check(who, *q);
}
int rs_op_band_hist(const uint8_t* tiles, const uint8_t* label_masks, const int32_t* tile_first, int n_tiles, int n_inst, int side,
                    int channels, uint32_t* hist, void* stream) {
  BandHistParams q;
  { int rc = band_hist_params("rs_op_band_hist", &q, tiles, label_masks, tile_first, n_tiles, n_inst, side, channels, hist); if (rc) return rc; }
  return launch_band_hist(q, (hipStream_t)stream);
}
int rs_host_band_hist(const uint8_t* tiles, const uint8_t* label_masks, const int32_t* tile_first, int n_tiles, int n_inst, int side,
                      int channels, uint32_t* hist) {
  BandHistParams q;
  { int rc = band_hist_params("rs_host_band_hist", &q, tiles, label_masks, tile_first, n_tiles, n_inst, side, channels, hist); if (rc) return rc; }
  return host_band_hist(q);
}

int rs_op_conv2d_dgrad(const void* dy, const void* w_t, void* dx, const void* res, const float* res32, const void* mask,
                       const void* down, int n, int hi, int wi, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                       int pad, int kpad, int halo, int variant, void* stream) {
  RS_CHECK(dy && w_t && dx, RS_ERR_ARG, "null argument");
  RS_CHECK(stride == 1 || (kh == 1 && kw == 1), RS_ERR_UNSUPPORTED, "dgrad: stride %d needs a 1x1 kernel (STRIDE_IN_1X1)", stride);
  RS_CHECK(halo >= kh - 1 - pad && halo >= 0 && kh == kw, RS_ERR_ARG, "dgrad: halo %d too small", halo);
  // the input gradient of conv(x, W, stride 1, pad) is conv(dy, W^T flipped, stride 1, pad' = k-1-pad); of a stride-s 1x1
  // convolution it is the 1x1 convolution of dy stored at every s-th pixel of dx
  ConvParams p;
  memset(&p, 0, sizeof p);
  const int pad_t = kh - 1 - pad;
  const int oh = stride == 1 ? ho + 2 * pad_t - kh + 1 : ho, ow = stride == 1 ? wo + 2 * pad_t - kw + 1 : wo;
  RS_CHECK(stride == 1 ? (oh == hi && ow == wi) : ((ho - 1) * stride < hi && (wo - 1) * stride < wi), RS_ERR_ARG, "dgrad: geometry");
  OpScratch scratch(stream);
  void* zero_bias = nullptr;
  { int rc = scratch.alloc(&zero_bias, (size_t)cin * 4 + 256); if (rc) return rc; }
  RS_HIP(hipMemsetAsync(zero_bias, 0, (size_t)cin * 4 + 256, (hipStream_t)stream));
  p.in = (const half_t*)dy; p.w = (const half_t*)w_t; p.bias = (const float*)zero_bias; p.out = dx;
  p.res = (const half_t*)res; p.res32 = res32; p.mask = (const half_t*)mask; p.down = (const half_t*)down;
  p.M = n * oh * ow; p.Ho = oh; p.Wo = ow;
  p.in_Hp = ho + 2 * halo; p.in_Wp = wo + 2 * halo; p.in_Cs = cout; p.in_off = halo - pad_t;
  p.stride = 1; p.KH = kh; p.KW = kw; p.Cin = cout; p.Kpad = kpad; p.Cout = cin;
  p.out_Hp = hi + 2 * halo; p.out_Wp = wi + 2 * halo; p.out_Cs = cin; p.out_pad = halo;
  p.out_stride = stride;
  if (down) { p.down_Hp = 2 * hi + 2 * halo; p.down_Wp = 2 * wi + 2 * halo; p.down_Cs = cin; p.down_pad = halo; }
  return launch_conv(p, (hipStream_t)stream, variant, 1);
}

// The same input gradient from fp32 tensors (dy, w_t [cin][kpad] transposed and tap-flipped, dx, res, mask, down: all float) with the product
// on the fp16 matrix cores: dY as hi + lo planes under one power-of-two scale per call, W^T as row-scaled planes, three products into one
// fp32 accumulator (conv_igemm's TRAIN && SPLIT instantiation).  Scratch, abs-max, planes and row split live for the call.  count_dev
// (optional, device): images computed = min(n, *count_dev); the others are not written.  Arguments are refused before a device is touched.
int rs_op_conv2d_dgrad_split(const void* dy, const void* w_t, void* dx, const void* res, const float* res32, const void* mask,
                             const void* down, int n, int hi, int wi, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                             int pad, int kpad, int halo, int variant, const int32_t* count_dev, void* stream) {
  RS_CHECK(dy && w_t && dx, RS_ERR_ARG, "rs_op_conv2d_dgrad_split: null operand");
  RS_CHECK(n >= 1, RS_ERR_ARG, "rs_op_conv2d_dgrad_split: n %d", n);
  RS_CHECK(cout >= 64 && cout % 64 == 0, RS_ERR_ARG, "rs_op_conv2d_dgrad_split: cout %d (the K side) must be a multiple of 64", cout);
  RS_CHECK(stride == 1 || (stride > 1 && kh == 1 && kw == 1), RS_ERR_UNSUPPORTED, "rs_op_conv2d_dgrad_split: stride %d needs a 1x1 kernel", stride);
  RS_CHECK(kh == kw && kh >= 1 && pad >= 0 && halo >= 0 && halo >= kh - 1 - pad, RS_ERR_ARG, "rs_op_conv2d_dgrad_split: halo %d below k - 1 - pad = %d", halo, kh - 1 - pad);
  RS_CHECK(hi >= 1 && wi >= 1 && ho >= 1 && wo >= 1 && cin >= 16 && cin % 16 == 0 && kpad >= kh * kw * cout && kpad % 64 == 0, RS_ERR_ARG,
           "rs_op_conv2d_dgrad_split: geometry (cin %d must be a multiple of 16, kpad %d at least kh * kw * cout and a multiple of 64)", cin, kpad);
  RS_CHECK(conv_dgrad_split_serves(cin, cout, kh, kw, stride), RS_ERR_UNSUPPORTED, "rs_op_conv2d_dgrad_split: shape not served");
  const int pad_t = kh - 1 - pad;
  const int oh = stride == 1 ? ho + 2 * pad_t - kh + 1 : ho, ow = stride == 1 ? wo + 2 * pad_t - kw + 1 : wo;
  RS_CHECK(stride == 1 ? (oh == hi && ow == wi) : ((ho - 1) * stride < hi && (wo - 1) * stride < wi), RS_ERR_ARG, "rs_op_conv2d_dgrad_split: geometry");
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.out = dx; p.res = (const half_t*)res; p.res32 = res32; p.mask = (const half_t*)mask; p.down = (const half_t*)down;
  p.M = n * oh * ow; p.Ho = oh; p.Wo = ow;
  p.in_Hp = ho + 2 * halo; p.in_Wp = wo + 2 * halo; p.in_Cs = cout; p.in_off = halo - pad_t;
  p.stride = 1; p.KH = kh; p.KW = kw; p.Cin = cout; p.Kpad = kpad; p.Cout = cin;
  p.out_Hp = hi + 2 * halo; p.out_Wp = wi + 2 * halo; p.out_Cs = cin; p.out_pad = halo;
  p.out_stride = stride;
  if (down) { p.down_Hp = 2 * hi + 2 * halo; p.down_Wp = 2 * wi + 2 * halo; p.down_Cs = cin; p.down_pad = halo; }
  if (count_dev) { p.m_count = count_dev; p.m_mul = oh * ow; }
  // one allocation: [dY header + planes | W^T planes | inverse row scales]
  const long long cap = (long long)n * p.in_Hp * p.in_Wp * cout;
  const size_t b_dy = (dgrad_split_scratch_bytes(cap) + 255) & ~(size_t)255, b_w = ((size_t)cin * kpad * 4 + 255) & ~(size_t)255;
  hipStream_t s = (hipStream_t)stream;
  OpScratch scratch(stream);
  char* buf = nullptr;
  { int rc = scratch.alloc((void**)&buf, b_dy + b_w + (size_t)cin * 4); if (rc) return rc; }
  p.in = (const half_t*)dy;
  { int rc = launch_dgrad_split_planes(p, buf, cap, s); if (rc) return rc; }
  SplitRowsDesc d = {(const float*)w_t, (half_t*)(buf + b_dy), (float*)(buf + b_dy + b_w), cin, kpad, 0u};
  { int rc = launch_split_rows(d, s); if (rc) return rc; }
  p.split = 1; p.dy_amax = (const unsigned*)buf;
  p.in = (const half_t*)(buf + WGS_HEAD_BYTES); p.in_lo = cap;
  p.w = d.planes; p.w_lo = (long long)cin * kpad; p.wscale = d.inv;
  return launch_conv(p, s, variant, 1);
}
// 1 when rs_op_conv2d_dgrad_split (and the trainer's split input-gradient mode) runs a layer of this shape on the fp16 matrix cores.  Host only.
int rs_op_conv2d_dgrad_split_serves(int cin, int cout, int kh, int stride) {
  return conv_dgrad_split_serves(cin, cout, kh, kh, stride) ? 1 : 0;
}
// The forward convolution / linear layer of the fp32 trainer from fp32 tensors (x, w [cout][kpad] in the engine's layout, bias, res, up, y:
// all float) with the product on the fp16 matrix cores: X as hi + lo planes under one power-of-two scale per call, W as row-scaled planes,
// three products into one fp32 accumulator (conv_igemm's TRAIN && SPLIT instantiation with the forward epilogue).  Scratch, abs-max,
// planes and row split live for the call.  count_dev (optional, device): images computed = min(n, *count_dev); the others are not written.
// Arguments are refused before a device is touched.
int rs_op_conv2d_fwd_split(const void* x, const void* w, const float* bias, void* y, const void* res, const void* up, int n, int hi, int wi,
                           int cin, int in_halo, int kh, int kw, int stride, int pad, int cout, int kpad, int out_halo, int relu, int variant,
                           const int32_t* count_dev, void* stream) {
  RS_CHECK(x && w && bias && y, RS_ERR_ARG, "rs_op_conv2d_fwd_split: null operand");
  RS_CHECK(n >= 1, RS_ERR_ARG, "rs_op_conv2d_fwd_split: n %d", n);
  RS_CHECK(cin >= 64 && cin % 64 == 0, RS_ERR_ARG, "rs_op_conv2d_fwd_split: cin %d (the K side) must be a multiple of 64", cin);
  RS_CHECK(cout >= 16 && cout % 16 == 0, RS_ERR_ARG, "rs_op_conv2d_fwd_split: cout %d (the rows) must be a multiple of 16", cout);
  RS_CHECK(kh == kw && kh >= 1 && stride >= 1 && pad >= 0 && out_halo >= 0 && in_halo >= pad, RS_ERR_ARG, "rs_op_conv2d_fwd_split: halo %d below the pad %d (or a kernel that is not square, stride %d)", in_halo, pad, stride);
  RS_CHECK(hi >= 1 && wi >= 1 && hi + 2 * pad >= kh && wi + 2 * pad >= kw && kpad >= kh * kw * cin && kpad % 64 == 0, RS_ERR_ARG,
           "rs_op_conv2d_fwd_split: geometry (%d x %d input, %dx%d kernel, kpad %d at least kh * kw * cin and a multiple of 64)", hi, wi, kh, kw, kpad);
  RS_CHECK(conv_fwd_split_serves(cout, cin, kh, kw, stride), RS_ERR_UNSUPPORTED, "rs_op_conv2d_fwd_split: shape not served");
  const int ho = (hi + 2 * pad - kh) / stride + 1, wo = (wi + 2 * pad - kw) / stride + 1;
  ConvParams p;
  memset(&p, 0, sizeof p);
  p.bias = bias; p.out = y; p.res = (const half_t*)res; p.up = (const half_t*)up;
  p.M = n * ho * wo; p.Ho = ho; p.Wo = wo;
  p.in_Hp = hi + 2 * in_halo; p.in_Wp = wi + 2 * in_halo; p.in_Cs = cin; p.in_off = in_halo - pad;
  p.stride = stride; p.KH = kh; p.KW = kw; p.Cin = cin; p.Kpad = kpad; p.Cout = cout;
  p.out_Hp = ho + 2 * out_halo; p.out_Wp = wo + 2 * out_halo; p.out_Cs = cout; p.out_pad = out_halo;
  if (up) { p.up_Hp = (ho + 1) / 2 + 2 * out_halo; p.up_Wp = (wo + 1) / 2 + 2 * out_halo; p.up_Cs = cout; p.up_pad = out_halo; }
  p.relu = relu ? 1 : 0;
  if (count_dev) { p.m_count = count_dev; p.m_mul = ho * wo; }
  // one allocation: [X header + planes | W planes | inverse row scales]
  const long long cap = (long long)n * p.in_Hp * p.in_Wp * cin;
  const size_t b_x = (dgrad_split_scratch_bytes(cap) + 255) & ~(size_t)255, b_w = ((size_t)cout * kpad * 4 + 255) & ~(size_t)255;
  hipStream_t s = (hipStream_t)stream;
  OpScratch scratch(stream);
  char* buf = nullptr;
  { int rc = scratch.alloc((void**)&buf, b_x + b_w + (size_t)cout * 4); if (rc) return rc; }
  p.in = (const half_t*)x;
  { int rc = launch_fwd_split_planes(p, buf, cap, s); if (rc) return rc; }
  SplitRowsDesc d = {(const float*)w, (half_t*)(buf + b_x), (float*)(buf + b_x + b_w), cout, kpad, 0u};
  { int rc = launch_split_rows(d, s); if (rc) return rc; }
  p.split = 1; p.x_amax = (const unsigned*)buf;
  p.in = (const half_t*)(buf + WGS_HEAD_BYTES); p.in_lo = cap;
  p.w = d.planes; p.w_lo = (long long)cout * kpad; p.wscale = d.inv;
  return launch_conv(p, s, variant, 1);
}
// 1 when rs_op_conv2d_fwd_split (and the trainer's split forward mode) runs a layer of this shape on the fp16 matrix cores.  Host only.
int rs_op_conv2d_fwd_split_serves(int cin, int cout, int k, int stride) {
  return conv_fwd_split_serves(cout, cin, k, k, stride) ? 1 : 0;
}
// w [rows][k] fp32 (device) -> planes [2 * rows][k] fp16 (hi rows, then lo rows) and inv_scale [rows], by weights.split_planes' rule
int rs_op_split_rows(const float* w, int rows, int k, void* planes, float* inv_scale, void* stream) {
  RS_CHECK(w && planes && inv_scale && rows >= 1 && k >= 1, RS_ERR_ARG, "rs_op_split_rows: bad argument");
  SplitRowsDesc d = {w, (half_t*)planes, inv_scale, rows, k, 0u};
  return launch_split_rows(d, (hipStream_t)stream);
}

static int op_conv2d_wgrad(const void* dy, const void* x, float* grad, const float* scale, int n, int hi, int wi, int cin, int in_halo,
                           int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits, void* stream, int f32);   // f32 = 2: split operands
int rs_op_conv2d_wgrad(const void* dy, const void* x, float* grad, const float* scale, int n, int hi, int wi, int cin, int in_halo,
                       int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits, void* stream) {
  return op_conv2d_wgrad(dy, x, grad, scale, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, dy_halo, splits, stream, 0);
}
// the same weight gradient from fp32 operands (reference-precision trainer: conv_wgrad_f32_kernel)
int rs_op_conv2d_wgrad_f32(const void* dy, const void* x, float* grad, const float* scale, int n, int hi, int wi, int cin, int in_halo,
                           int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits, void* stream) {
  return op_conv2d_wgrad(dy, x, grad, scale, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, dy_halo, splits, stream, 1);
}
// the fp32 weight gradient with the product on the fp16 matrix cores (hi + lo planes of the scaled operands: conv_wgrad_split_kernel);
// the plane scratch lives for the call.  Arguments are refused before a device is touched.
int rs_op_conv2d_wgrad_split(const void* dy, const void* x, float* grad, const float* scale, int n, int hi, int wi, int cin, int in_halo,
                             int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits, void* stream) {
  RS_CHECK(dy && x && grad, RS_ERR_ARG, "rs_op_conv2d_wgrad_split: null operand");
  RS_CHECK(n >= 1 && hi >= 1 && wi >= 1 && kh >= 1 && kw >= 1 && stride >= 1 && pad >= 0 && in_halo >= pad && dy_halo >= 0 && hi + 2 * pad >= kh &&
           wi + 2 * pad >= kw, RS_ERR_ARG, "rs_op_conv2d_wgrad_split: geometry (%d x %d x %d input, %dx%d kernel, stride %d, pad %d, halos %d / %d)",
           n, hi, wi, kh, kw, stride, pad, in_halo, dy_halo);
  RS_CHECK(cin >= 64 && cin % 64 == 0 && cout >= 1 && cout % 4 == 0 && kpad == kh * kw * cin, RS_ERR_ARG,
           "rs_op_conv2d_wgrad_split: cin %d must be a multiple of 64, cout %d of 4, and kpad %d = kh * kw * cin", cin, cout, kpad);
  return op_conv2d_wgrad(dy, x, grad, scale, n, hi, wi, cin, in_halo, kh, kw, stride, pad, cout, kpad, dy_halo, splits, stream, 2);
}
// 1 when rs_op_conv2d_wgrad_split (and the trainer's split mode) runs this layer on the fp16 matrix cores, 0 when it falls through to the
// fp32 kernel (gradient rows or inputs whose channel count is no multiple of 8).  Host only.
int rs_op_conv2d_wgrad_split_serves(int cin, int cout) {
  WgradParams p;
  memset(&p, 0, sizeof p);
  p.f32 = 1; p.Cin = cin; p.in_Cs = cin; p.Cout = cout; p.dy_Cs = cout;
  return cin >= 64 && cout >= 1 && wgrad_split_serves(p) ? 1 : 0;
}
static int op_conv2d_wgrad(const void* dy, const void* x, float* grad, const float* scale, int n, int hi, int wi, int cin, int in_halo,
                           int kh, int kw, int stride, int pad, int cout, int kpad, int dy_halo, int splits, void* stream, int f32) {
  RS_CHECK(dy && x && grad, RS_ERR_ARG, "null argument");
  RS_CHECK(in_halo >= pad, RS_ERR_ARG, "input halo %d < pad %d", in_halo, pad);
  const int ho = (hi + 2 * pad - kh) / stride + 1, wo = (wi + 2 * pad - kw) / stride + 1;
  WgradParams p;
  memset(&p, 0, sizeof p);
  p.dy = (const half_t*)dy; p.x = (const half_t*)x; p.grad = grad; p.scale = scale;
  p.M = n * ho * wo; p.Ho = ho; p.Wo = wo;
  p.dy_Hp = ho + 2 * dy_halo; p.dy_Wp = wo + 2 * dy_halo; p.dy_Cs = cout; p.dy_pad = dy_halo;
  p.in_Hp = hi + 2 * in_halo; p.in_Wp = wi + 2 * in_halo; p.in_Cs = cin; p.in_off = in_halo - pad;
  p.stride = stride; p.KH = kh; p.KW = kw; p.Cin = cin; p.Cout = cout; p.Kpad = kpad;
  p.f32 = f32 ? 1 : 0;
  p.split_ops = f32 == 2;
  p.splits = splits > 0 ? splits : wgrad_splits(p);
  hipStream_t s = (hipStream_t)stream;
  OpScratch scratch(stream);
  void *partial = nullptr, *zeros = nullptr;
  { int rc = scratch.alloc(&partial, (size_t)p.splits * cout * kpad * 4); if (rc) return rc; }
  // split operands: the header (with its zero row) and the planes come before the fp16 kernel's zero row in the same allocation
  size_t planes = 0;
  if (p.split_ops) {
    p.split_dy_cap = (long long)n * p.dy_Hp * p.dy_Wp * p.dy_Cs;
    p.split_x_cap = (long long)n * p.in_Hp * p.in_Wp * p.in_Cs;
    planes = (wgrad_split_scratch_bytes(p.split_dy_cap, p.split_x_cap) + 255) & ~(size_t)255;
  }
  { int rc = scratch.alloc(&zeros, planes + (size_t)cout * 2 + 256); if (rc) return rc; }
  if (p.split_ops) {
    p.split_scratch = zeros;
    RS_HIP(hipMemsetAsync(zeros, 0, WGS_HEAD_BYTES, s));
    zeros = (char*)zeros + planes;
  }
  RS_HIP(hipMemsetAsync(zeros, 0, (size_t)cout * 2 + 256, s));
  RS_HIP(hipMemsetAsync(partial, 0, (size_t)p.splits * cout * kpad * 4, s));   // K padding columns stay zero
  p.partial = (float*)partial; p.zeros = (const half_t*)zeros;
  return launch_conv_wgrad(p, s);
}

// backward of the stem's max-pool fused with its ReLU mask (stem_bwd.hip)
int rs_op_maxpool3x3s2_bwd(const void* x, const void* dq, void* dx, int n, int hc, int wc, int c, int x_halo, int q_halo, int f32, void* stream) {
  RS_CHECK(x && dq && dx, RS_ERR_ARG, "rs_op_maxpool3x3s2_bwd: null operand");
  RS_CHECK(n >= 1 && hc >= 1 && wc >= 1 && c >= 1 && x_halo >= 0 && q_halo >= 0, RS_ERR_ARG,
           "rs_op_maxpool3x3s2_bwd: geometry (%d x %d x %d x %d, halos %d / %d)", n, hc, wc, c, x_halo, q_halo);
  PoolBwdParams p;
  memset(&p, 0, sizeof p);
  p.x = x; p.dq = dq; p.dx = dx;
  p.N = n; p.Hc = hc; p.Wc = wc; p.Hq = (hc - 1) / 2 + 1; p.Wq = (wc - 1) / 2 + 1; p.C = c; p.x_halo = x_halo; p.q_halo = q_halo;
  p.f32 = f32 ? 1 : 0;
  return launch_maxpool3x3s2_bwd(p, (hipStream_t)stream);
}
// weight gradient of the stem convolution in its forward GEMM layout (stem_bwd.hip); the partial sums live for the call
static int op_stem_wgrad(const void* dy, const void* x0, float* grad, const float* scale, int n, int hc, int wc, int cin, int dy_halo,
                         int x_halo, int splits, void* stream, int f32) {
  RS_CHECK(dy && x0 && grad, RS_ERR_ARG, "rs_op_stem_wgrad: null operand");
  RS_CHECK(n >= 1 && hc >= 1 && wc >= 1 && (long long)n * hc * wc < (1ll << 31) - 8 && 4 / wc < hc, RS_ERR_ARG, "rs_op_stem_wgrad: %d x %d x %d pixels", n, hc, wc);
  RS_CHECK(cin >= 1 && cin <= 4 && dy_halo >= 0 && x_halo >= 3, RS_ERR_ARG, "rs_op_stem_wgrad: %d input channels of 4, halos %d / %d (input: at least 3)", cin, dy_halo, x_halo);
  RS_CHECK(splits <= RS_STEM_WGRAD_MAX_SPLITS, RS_ERR_ARG, "rs_op_stem_wgrad: %d splits, at most %d", splits, RS_STEM_WGRAD_MAX_SPLITS);
  StemWgradParams p;
  memset(&p, 0, sizeof p);
  p.dy = dy; p.x0 = x0; p.scale = scale; p.grad = grad;
  p.N = n; p.Hc = hc; p.Wc = wc; p.dy_halo = dy_halo; p.x_halo = x_halo; p.cin = cin;
  p.splits = splits > 0 ? splits : stem_wgrad_splits((long long)n * hc * wc);
  p.f32 = f32;
  OpScratch scratch(stream);
  { int rc = scratch.alloc((void**)&p.partial, (size_t)p.splits * 64 * RS_STEM_KPAD * 4); if (rc) return rc; }
  return launch_stem_wgrad(p, (hipStream_t)stream);
}
int rs_op_stem_wgrad(const void* dy, const void* x0, float* grad, const float* scale, int n, int hc, int wc, int cin, int dy_halo,
                     int x_halo, int splits, void* stream) {
  return op_stem_wgrad(dy, x0, grad, scale, n, hc, wc, cin, dy_halo, x_halo, splits, stream, 0);
}
int rs_op_stem_wgrad_f32(const void* dy, const void* x0, float* grad, const float* scale, int n, int hc, int wc, int cin, int dy_halo,
                         int x_halo, int splits, void* stream) {
  return op_stem_wgrad(dy, x0, grad, scale, n, hc, wc, cin, dy_halo, x_halo, splits, stream, 1);
}

int rs_op_nms(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep, int segments, int cap,
              float thresh, void* stream) {
  RS_CHECK(boxes && counts && keep && segments > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(cap >= 1 && cap <= 2048, RS_ERR_ARG, "cap %d outside [1,2048]", cap);
  NmsParams p = {};
  p.boxes = boxes; p.count = counts; p.valid = valid; p.keep = keep; p.cap = cap; p.thresh = thresh;
  OpScratch scratch(stream);
  // the engine's dispatch: training capacity always keeps the suppression mask in global memory; at cap <= 1024 the engine passes
  // scratch too, and launch_nms takes the global-memory form for <= 32 segments, the LDS form above that
  if (cap > 1024) {
    int rc = scratch.alloc((void**)&p.scratch, (size_t)segments * 2048 * 32 * 8);
    if (rc) return rc;
  } else if (segments <= 32) {
    int rc = scratch.alloc((void**)&p.scratch, (size_t)segments * 1024 * 16 * 8);
    if (rc) return rc;
  }
  return launch_nms(p, segments, (hipStream_t)stream);
}

int rs_op_batched_nms(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep, int images, int segments_per_image,
                      int cap, float thresh, int rule, void* stream) {
  return rs_op_batched_nms_decision(boxes, counts, valid, keep, images, segments_per_image, cap, thresh, rule, nullptr, nullptr, stream);
}

int rs_op_batched_nms_decision(const float* boxes, const int32_t* counts, const uint8_t* valid, uint8_t* keep, int images, int segments_per_image,
                               int cap, float thresh, int rule, int32_t* rule_out, float* unit_out, void* stream) {
  RS_CHECK(boxes && counts && keep && images > 0 && segments_per_image > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(cap >= 1 && cap <= 2048, RS_ERR_ARG, "cap %d outside [1,2048]", cap);
  RS_CHECK(rule == 0 || rule == 1, RS_ERR_ARG, "rule %d (0 = per category, 1 = torchvision's size rule)", rule);
  const int segments = images * segments_per_image;
  RS_CHECK(rule || (!rule_out && !unit_out), RS_ERR_ARG, "rule 0 takes no decision");
  if (!rule) return rs_op_nms(boxes, counts, valid, keep, segments, cap, thresh, stream);
  RS_CHECK(cap > 1000, RS_ERR_ARG, "cap %d: the size rule needs a capacity above 1000 boxes per segment", cap);
  hipStream_t s = (hipStream_t)stream;
  NmsParams p = {};
  p.boxes = boxes; p.count = counts; p.valid = valid; p.keep = keep; p.cap = cap; p.thresh = thresh;
  OpScratch scratch(stream);
  void* dec = nullptr;
  { int rc = scratch.alloc(&dec, (size_t)images * 12); if (rc) return rc; }
  // the suppression mask as in rs_op_nms (= the engine's dispatch)
  const size_t sbytes = cap > 1024 ? (size_t)segments * 2048 * 32 * 8 : (segments <= 32 ? (size_t)segments * 1024 * 16 * 8 : 0);
  if (sbytes) { int rc = scratch.alloc((void**)&p.scratch, sbytes); if (rc) return rc; }
  p.rule = (int*)dec; p.unit = (float*)((char*)dec + (size_t)images * 8); p.group = segments_per_image;
  int rc = launch_nms(p, segments, s);
  // the decision as nms_kernel's prologue left it (the engine's rpn_nms_rule / rpn_nms_unit tensors)
  if (!rc && rule_out && hipMemcpyAsync(rule_out, p.rule, (size_t)images * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = RS_ERR_HIP;
  if (!rc && unit_out && hipMemcpyAsync(unit_out, p.unit, (size_t)images * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = RS_ERR_HIP;
  return rc;
}

int rs_op_det_merge(const float* dec_boxes, const float* dec_scores, const int32_t* seg_roi, const int32_t* seg_count, const uint8_t* keep,
                    int images, int num_classes, int cap, int dets_per_image, float scale_x, float scale_y, float out_w, float out_h,
                    float* det_boxes_net, float* det_boxes, float* det_scores, int32_t* det_classes, int32_t* det_roi, int32_t* det_count,
                    void* stream) {
  RS_CHECK(dec_boxes && dec_scores && seg_roi && seg_count && keep && det_boxes_net && det_boxes && det_scores && det_classes && det_count &&
               images > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(num_classes >= 1 && num_classes <= RS_MAX_CLASSES, RS_ERR_UNSUPPORTED, "NUM_CLASSES %d outside [1,%d]", num_classes, RS_MAX_CLASSES);
  RS_CHECK(cap >= 1 && cap <= 1024, RS_ERR_ARG, "cap %d outside [1,1024]", cap);
  { const int rc0 = det_merge_check(num_classes, dets_per_image); if (rc0) return rc0; }
  hipStream_t s = (hipStream_t)stream;
  DetMergeParams p;
  memset(&p, 0, sizeof p);
  p.dec_boxes = dec_boxes; p.dec_scores = dec_scores; p.seg_roi = seg_roi; p.seg_count = seg_count; p.keep = keep;
  p.K = num_classes; p.cap = cap; p.dets_per_image = dets_per_image;
  p.scale_x = scale_x; p.scale_y = scale_y; p.out_w = out_w; p.out_h = out_h;
  p.det_boxes_net = det_boxes_net; p.det_boxes = det_boxes; p.det_scores = det_scores; p.det_classes = det_classes; p.det_roi = det_roi;
  p.det_count = det_count;
  OpScratch scratch(stream);
  if (num_classes > RS_DET_GROUP) {    // the partial winners between the two launches, for the time of this call (the engine owns its own)
    const size_t G = (size_t)det_merge_groups(num_classes);
    const size_t kb = (size_t)images * G * dets_per_image * 8;
    void* ws = nullptr;
    { int rc = scratch.alloc(&ws, kb + (size_t)images * G * 4); if (rc) return rc; }
    p.part_keys = (unsigned long long*)ws; p.part_count = (int*)((char*)ws + kb);
  }
  return launch_det_merge(p, images, s);
}

int rs_op_roi_align(const void* const feats[4], const int32_t heights[4], const int32_t widths[4], const float scales[4],
                    int nlevels, const float* rois, int n_rois, int rois_per_image, int P, int out_halo, void* out,
                    int32_t* levels_out, void* stream) {
  RS_CHECK(feats && rois && out && nlevels >= 1 && nlevels <= 4 && n_rois > 0 && rois_per_image > 0, RS_ERR_ARG, "bad argument");
  RoiAlignParams p;
  memset(&p, 0, sizeof p);
  for (int l = 0; l < nlevels; ++l) { p.feat[l] = (const half_t*)feats[l]; p.H[l] = heights[l]; p.W[l] = widths[l]; p.scale[l] = scales[l]; }
  p.nlevels = nlevels; p.C = 256; p.rois = rois; p.S = n_rois; p.slots_per_image = rois_per_image;
  p.out = (half_t*)out; p.P = P; p.out_pad = out_halo; p.out_level = levels_out;
  rs_debug_reload();                                         // RS_ROI_WINDOW: the operator tests switch between the two forward forms
  return launch_roi_align(p, (hipStream_t)stream);
}

int rs_op_roi_align_bwd(float* const dfeats[4], const int32_t heights[4], const int32_t widths[4], const float scales[4],
                        int nlevels, const float* rois, int n_rois, int rois_per_image, int P, int out_halo, const void* dout,
                        void* stream) {
  RS_CHECK(dfeats && rois && dout && nlevels >= 1 && nlevels <= 4 && n_rois > 0 && rois_per_image > 0, RS_ERR_ARG, "bad argument");
  RoiAlignParams p;
  memset(&p, 0, sizeof p);
  for (int l = 0; l < nlevels; ++l) { p.dfeat[l] = dfeats[l]; p.H[l] = heights[l]; p.W[l] = widths[l]; p.scale[l] = scales[l]; }
  p.nlevels = nlevels; p.C = 256; p.rois = rois; p.S = n_rois; p.slots_per_image = rois_per_image;
  p.out = (half_t*)dout; p.P = P; p.out_pad = out_halo;
  rs_debug_reload();                                         // RS_ROI_BWD_ATOMIC: the operator tests switch between the two forms
  // workspace of the owner-computes form (the trainer owns its own): per-entry tables + the overflow counter, for the time of this call
  p.n_images = (n_rois + rois_per_image - 1) / rois_per_image;
  OpScratch scratch(stream);
  void* ws = nullptr;
  { int rc = scratch.alloc(&ws, (size_t)n_rois * RS_ROI_BWD_TABLE_BYTES + 64); if (rc) return rc; }
  p.bwd_overflow = (int*)ws;
  p.bwd_tables = (char*)ws + 64;
  const int rc = launch_roi_align_bwd(p, (hipStream_t)stream);
  RS_HIP(scratch.sync());
  return rc;
}

// The two operators above with everything the engine and the trainer put into RoiAlignParams: precision, compact entries, per-image
// counts, the visiting order, the gradient's storage type.  Same launchers; tests/test_gpu_roi_bounds.py reaches every kernel form here.
int rs_op_roi_align_form(const void* const feats[4], const int64_t feat_lo[4], const int32_t heights[4], const int32_t widths[4],
                         const float scales[4], int nlevels, const float* rois, int n_entries_cap, int slots_per_image, int P, int out_halo,
                         int precision, void* out, int64_t out_lo, const int32_t* slot_list, const int32_t* n_entries,
                         const int32_t* per_image_count, const int32_t* order, int32_t* levels_out, void* stream) {
  RS_CHECK(feats && rois && out && nlevels >= 1 && nlevels <= 4 && n_entries_cap > 0 && slots_per_image > 0, RS_ERR_ARG, "bad argument");
  RS_CHECK(precision >= 0 && precision <= 2 && (precision != 2 || feat_lo), RS_ERR_ARG, "precision %d (0 fp16, 1 fp32, 2 split with feat_lo)", precision);
  RoiAlignParams p;
  memset(&p, 0, sizeof p);
  for (int l = 0; l < nlevels; ++l) {
    p.feat[l] = (const half_t*)feats[l]; p.H[l] = heights[l]; p.W[l] = widths[l]; p.scale[l] = scales[l];
    if (precision == 2) p.feat_lo[l] = feat_lo[l];
  }
  p.nlevels = nlevels; p.C = 256; p.rois = rois; p.S = n_entries_cap; p.slots_per_image = slots_per_image;
  p.slot_list = slot_list; p.n_entries = n_entries; p.per_image_count = per_image_count; p.order = order;
  p.out = (half_t*)out; p.P = P; p.out_pad = out_halo; p.out_level = levels_out;
  p.f32 = precision; p.out_lo = precision == 2 ? out_lo : 0;
  rs_debug_reload();                                         // RS_ROI_WINDOW
  return launch_roi_align(p, (hipStream_t)stream);
}

int rs_op_roi_align_bwd_form(float* const dfeats[4], const int32_t heights[4], const int32_t widths[4], const float scales[4], int nlevels,
                             const float* rois, int n_entries_cap, int slots_per_image, int n_images, int P, int out_halo, int grad_f32,
                             const void* dout, const int32_t* slot_list, const int32_t* n_entries, const int32_t* per_image_count,
                             void* stream) {
  RS_CHECK(dfeats && rois && dout && nlevels >= 1 && nlevels <= 4 && n_entries_cap > 0 && slots_per_image > 0 && n_images > 0, RS_ERR_ARG,
           "bad argument");
  RoiAlignParams p;
  memset(&p, 0, sizeof p);
  for (int l = 0; l < nlevels; ++l) { p.dfeat[l] = dfeats[l]; p.H[l] = heights[l]; p.W[l] = widths[l]; p.scale[l] = scales[l]; }
  p.nlevels = nlevels; p.C = 256; p.rois = rois; p.S = n_entries_cap; p.slots_per_image = slots_per_image;
  p.slot_list = slot_list; p.n_entries = n_entries; p.per_image_count = per_image_count;
  p.out = (half_t*)dout; p.P = P; p.out_pad = out_halo; p.f32 = grad_f32 ? 1 : 0;
  rs_debug_reload();                                         // RS_ROI_BWD_ATOMIC
  p.n_images = n_images;
  OpScratch scratch(stream);
  void* ws = nullptr;
  { int rc = scratch.alloc(&ws, (size_t)n_entries_cap * RS_ROI_BWD_TABLE_BYTES + 64); if (rc) return rc; }
  p.bwd_overflow = (int*)ws;
  p.bwd_tables = (char*)ws + 64;
  const int rc = launch_roi_align_bwd(p, (hipStream_t)stream);
  RS_HIP(scratch.sync());
  return rc;
}

int rs_op_rpn_loss(const float* head, void* dhead, const int32_t* labels, const float* anchors, const float* matched_gt,
                   float* loss_out, int n, int hw, int num_anchors, int cs, int level_off, int total_anchors, float normalizer,
                   float loss_scale, void* stream) {
  RpnLossParams p;
  memset(&p, 0, sizeof p);
  p.head = head; p.dhead = (half_t*)dhead; p.labels = labels; p.anchors = anchors; p.matched_gt = matched_gt; p.loss_out = loss_out;
  p.A = num_anchors; p.cs = cs; p.HW = hw; p.n_anchors = hw * num_anchors; p.level_off = level_off; p.total_anchors = total_anchors;
  p.normalizer = normalizer; p.loss_scale = loss_scale;
  return launch_rpn_loss(p, n, (hipStream_t)stream);
}

int rs_op_box_loss(const float* pred, void* dpred, const int32_t* gt_classes, const float* proposals, const float* gt_boxes,
                   float* loss_out, int n_rois, int num_classes, int cs, float n_valid, const float reg_weights[4], float loss_scale,
                   void* stream) {
  RS_CHECK(reg_weights, RS_ERR_ARG, "null argument");
  BoxLossParams p;
  memset(&p, 0, sizeof p);
  p.pred = pred; p.dpred = (half_t*)dpred; p.gt_classes = gt_classes; p.proposals = proposals; p.gt_boxes = gt_boxes; p.loss_out = loss_out;
  p.n_rois = n_rois; p.K = num_classes; p.cs = cs; p.n_valid = n_valid;
  p.wx = reg_weights[0]; p.wy = reg_weights[1]; p.ww = reg_weights[2]; p.wh = reg_weights[3]; p.loss_scale = loss_scale;
  return launch_box_loss(p, (hipStream_t)stream);
}

int rs_op_mask_loss(const float* logits, void* dlogits, const uint8_t* targets, const int32_t* gt_classes, float* loss_out, int n_masks,
                    int side, int cs, float loss_scale, void* stream) {
  MaskLossParams p;
  memset(&p, 0, sizeof p);
  p.logits = logits; p.dlogits = (half_t*)dlogits; p.targets = targets; p.gt_classes = gt_classes; p.loss_out = loss_out;
  p.n_masks = n_masks; p.S = side; p.cs = cs; p.loss_scale = loss_scale;
  return launch_mask_loss(p, (hipStream_t)stream);
}

// ---- training diagnostics: the three counting kernels on caller-owned device buffers, and the same rules (train_stats.h) on host
// pointers.  Both forms ADD into the counts and refuse null pointers and impossible geometry before anything is touched.
static int stats_label_args(const char* who, const int32_t* labels, int64_t count, const int32_t* counts2) {
  RS_CHECK(labels && counts2, RS_ERR_ARG, "%s: null argument", who);
  RS_CHECK(count >= 0, RS_ERR_ARG, "%s: negative count", who);
  RS_CHECK(count < (1ll << 31), RS_ERR_UNSUPPORTED, "%s: %lld labels do not fit a 32-bit count", who, (long long)count);
  return RS_OK;
}
static int stats_box_args(const char* who, const float* pred, const int32_t* gt_classes, int n_rois, int num_classes, int cs, int n_images,
                          const int32_t* counts7) {
  RS_CHECK(pred && gt_classes && counts7, RS_ERR_ARG, "%s: null argument", who);
  RS_CHECK(n_rois >= 0 && n_images >= 0, RS_ERR_ARG, "%s: negative count", who);
  RS_CHECK(num_classes >= 1 && num_classes <= TS_MAX_CLASSES && 5 * num_classes + 1 <= cs, RS_ERR_ARG,
           "%s: %d classes (1..%d) in rows of %d (at least 5K+1)", who, num_classes, TS_MAX_CLASSES, cs);
  return RS_OK;
}
static int stats_mask_args(const char* who, const float* logits, const uint8_t* targets, const int32_t* gt_classes, int n_masks, int side, int cs,
                           const int32_t* counts5) {
  RS_CHECK(logits && targets && gt_classes && counts5, RS_ERR_ARG, "%s: null argument", who);
  RS_CHECK(n_masks >= 0 && side >= 1 && cs >= 1, RS_ERR_ARG, "%s: %d entries of side %d in rows of %d", who, n_masks, side, cs);
  RS_CHECK((long long)n_masks * side * side < (1ll << 31), RS_ERR_UNSUPPORTED, "%s: %d entries of %d x %d pixels do not fit a 32-bit count", who,
           n_masks, side, side);
  return RS_OK;
}

int rs_op_label_counts(const int32_t* labels, int64_t count, int32_t* counts2, void* stream) {
  { int rc = stats_label_args("rs_op_label_counts", labels, count, counts2); if (rc) return rc; }
  LabelCountsParams p;
  memset(&p, 0, sizeof p);
  p.labels = labels; p.count = (int)count; p.out = counts2;
  return launch_label_counts(p, (hipStream_t)stream);
}
int rs_op_box_stats(const float* pred, const int32_t* gt_classes, int n_rois, int num_classes, int cs, const int32_t* sampled_counts,
                    int n_images, int32_t* counts7, void* stream) {
  { int rc = stats_box_args("rs_op_box_stats", pred, gt_classes, n_rois, num_classes, cs, n_images, counts7); if (rc) return rc; }
  BoxStatsParams p;
  memset(&p, 0, sizeof p);
  p.pred = pred; p.gt_classes = gt_classes; p.sampled_counts = sampled_counts; p.out = counts7;
  p.n_rois = n_rois; p.K = num_classes; p.cs = cs; p.n_images = n_images;
  return launch_box_stats(p, (hipStream_t)stream);
}
int rs_op_mask_stats(const float* logits, const uint8_t* targets, const int32_t* gt_classes, const int32_t* n_masks_ptr, int n_masks, int side,
                     int cs, int32_t* counts5, void* stream) {
  { int rc = stats_mask_args("rs_op_mask_stats", logits, targets, gt_classes, n_masks, side, cs, counts5); if (rc) return rc; }
  MaskStatsParams p;
  memset(&p, 0, sizeof p);
  p.logits = logits; p.targets = targets; p.gt_classes = gt_classes; p.n_masks_ptr = n_masks_ptr; p.out = counts5;
  p.n_masks = n_masks; p.S = side; p.cs = cs;
  return launch_mask_stats(p, (hipStream_t)stream);
}

int rs_host_label_counts(const int32_t* labels, int64_t count, int32_t* counts2) {
  { int rc = stats_label_args("rs_host_label_counts", labels, count, counts2); if (rc) return rc; }
  for (int64_t i = 0; i < count; ++i) {
    counts2[0] += labels[i] == 1;
    counts2[1] += labels[i] == 0;
  }
  return RS_OK;
}
int rs_host_box_stats(const float* pred, const int32_t* gt_classes, int n_rois, int num_classes, int cs, const int32_t* sampled_counts,
                      int n_images, int32_t* counts7) {
  { int rc = stats_box_args("rs_host_box_stats", pred, gt_classes, n_rois, num_classes, cs, n_images, counts7); if (rc) return rc; }
  if (sampled_counts)
    for (int i = 0; i < n_images; ++i) {
      counts7[0] += sampled_counts[2 * i];
      counts7[1] += sampled_counts[2 * i + 1];
    }
  for (int r = 0; r < n_rois; ++r) {
    int f[5];
    ts_box_row(pred + (size_t)r * cs, gt_classes[r], num_classes, f);
    for (int c = 0; c < 5; ++c) counts7[2 + c] += f[c];
  }
  return RS_OK;
}
int rs_host_mask_stats(const float* logits, const uint8_t* targets, const int32_t* gt_classes, const int32_t* n_masks_ptr, int n_masks, int side,
                       int cs, int32_t* counts5) {
  { int rc = stats_mask_args("rs_host_mask_stats", logits, targets, gt_classes, n_masks, side, cs, counts5); if (rc) return rc; }
  int n = n_masks;
  if (n_masks_ptr && *n_masks_ptr < n) n = *n_masks_ptr;
  const size_t per = (size_t)side * side;
  for (int m = 0; m < n; ++m) {
    const int cls = gt_classes[m];
    if (!ts_mask_entry_counts(cls, cs)) continue;
    for (size_t pix = 0; pix < per; ++pix) {
      int f[5];
      ts_mask_pixel(logits[((size_t)m * per + pix) * cs + cls], targets[(size_t)m * per + pix], f);
      for (int c = 0; c < 5; ++c) counts5[c] += f[c];
    }
  }
  return RS_OK;
}

int rs_op_match(const float* boxes, int per_image_boxes, const int32_t* box_count, const float* gt, const int32_t* gt_count,
                int32_t* matched, int32_t* labels, float* best_iou, int n_images, int n_boxes, int gt_cap, float t_lo, float t_hi,
                int lbl_lo, int lbl_mid, int lbl_hi, int allow_low_quality, void* stream) {
  MatchParams p;
  memset(&p, 0, sizeof p);
  p.boxes = boxes; p.per_image_boxes = per_image_boxes; p.box_count = box_count; p.gt = gt; p.gt_count = gt_count;
  p.matched = matched; p.labels = labels; p.best_iou = best_iou; p.n_boxes = n_boxes; p.gt_cap = gt_cap;
  p.t_lo = t_lo; p.t_hi = t_hi; p.lbl_lo = lbl_lo; p.lbl_mid = lbl_mid; p.lbl_hi = lbl_hi;
  OpScratch scratch(stream);
  if (allow_low_quality) {
    int rc = scratch.alloc((void**)&p.gt_best, (size_t)n_images * gt_cap * 4);
    if (rc) return rc;
  }
  return launch_match(p, n_images, (hipStream_t)stream);
}

int rs_op_subsample(int32_t* labels, int32_t* sampled, int32_t* sampled_count, int n_images, int n, int num_samples,
                    float positive_fraction, int bg_label, int rpn_mode, uint32_t seed, void* stream) {
  SubsampleParams p;
  memset(&p, 0, sizeof p);
  p.labels = labels; p.sampled = sampled; p.sampled_count = sampled_count; p.n = n; p.num_samples = num_samples;
  p.positive_fraction = positive_fraction; p.bg_label = bg_label; p.rpn_mode = rpn_mode; p.seed = seed;
  return launch_subsample(p, n_images, (hipStream_t)stream);
}

int rs_op_sgd_momentum(float* w, float* momentum_buf, const float* grad, int64_t n, float lr, float momentum, float weight_decay,
                       float inv_loss_scale, int first_step, void* stream) {
  return launch_sgd_momentum(w, momentum_buf, grad, n, lr, momentum, weight_decay, inv_loss_scale, first_step, (hipStream_t)stream);
}

// ---- the optimiser step over a table of segments (sgd_rule.h): the kernels on caller-owned device buffers, and the same rule on host
// pointers.  Both refuse a bad table or solver before anything is touched.
static int sgd_segments_args(const char* who, const void* w, const void* buf, const void* grad, int64_t n, const rs_solver* solver, bool device) {
  RS_CHECK(w && buf && grad, RS_ERR_ARG, "%s: null buffer", who);
  RS_CHECK(n > 0, RS_ERR_ARG, "%s: %lld values", who, (long long)n);
  RS_CHECK(!device || (((uintptr_t)w & 15) == 0 && ((uintptr_t)buf & 15) == 0 && ((uintptr_t)grad & 15) == 0), RS_ERR_ARG, "%s: the buffers must be 16-byte aligned", who);
  return sgd_solver_check(who, solver);
}

int rs_op_sgd_segments(float* w, float* momentum_buf, const float* grad, int64_t n, const int64_t* seg_off, const int64_t* seg_count,
                       const int32_t* seg_flags, int n_seg, float lr, float momentum, float weight_decay, float inv_scale,
                       const rs_solver* solver, const int32_t* skip, float* norms_out, float* coef_out, void* stream) {
  const char* who = "rs_op_sgd_segments";
  { int rc = sgd_segments_args(who, w, momentum_buf, grad, n, solver, true); if (rc) return rc; }
  SgdHyper h;
  int norm_inf = 0;
  { int rc = sgd_solver_hyper(who, *solver, lr, momentum, weight_decay, inv_scale, &h, &norm_inf); if (rc) return rc; }
  std::vector<SgdChunk> chunks;
  std::vector<int> seg_chunks;
  std::vector<uint8_t> host;
  { int rc = sgd_plan_cut(who, seg_off, seg_count, seg_flags, n_seg, n, &chunks, &seg_chunks); if (rc) return rc; }
  sgd_plan_pack(chunks, seg_chunks, &host);
  OpScratch scratch(stream);       // declared behind `host`: it waits for the stream before the staging vector goes
  void* base = nullptr;
  { int rc = scratch.alloc(&base, sgd_plan_bytes((int)chunks.size(), n_seg)); if (rc) return rc; }
  SgdPlan p = sgd_plan_place(base, (int)chunks.size(), n_seg);
  RS_HIP(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
  if (norms_out) p.norms = norms_out;
  if (coef_out) p.coef = coef_out;
  if (h.clip_type >= SGD_CLIP_NORM) {
    int rc = launch_grad_norms(p, grad, h, norm_inf, nullptr, (hipStream_t)stream);
    if (rc) return rc;
  }
  { int rc = launch_sgd_segments(p, w, momentum_buf, grad, h, skip, (hipStream_t)stream); if (rc) return rc; }
  RS_HIP(scratch.sync());
  return RS_OK;
}

int rs_host_sgd_segments(float* w, float* momentum_buf, const float* grad, int64_t n, const int64_t* seg_off, const int64_t* seg_count,
                         const int32_t* seg_flags, int n_seg, float lr, float momentum, float weight_decay, float inv_scale,
                         const rs_solver* solver, const int32_t* skip, float* norms_out, float* coef_out) {
  const char* who = "rs_host_sgd_segments";
  { int rc = sgd_segments_args(who, w, momentum_buf, grad, n, solver, false); if (rc) return rc; }
  SgdHyper h;
  int norm_inf = 0;
  { int rc = sgd_solver_hyper(who, *solver, lr, momentum, weight_decay, inv_scale, &h, &norm_inf); if (rc) return rc; }
  std::vector<SgdChunk> chunks;
  std::vector<int> seg_chunks;
  { int rc = sgd_plan_cut(who, seg_off, seg_count, seg_flags, n_seg, n, &chunks, &seg_chunks); if (rc) return rc; }
  std::vector<float> coef((size_t)n_seg, 1.f);
  if (h.clip_type >= SGD_CLIP_NORM) {
    std::vector<double> sums((size_t)n_seg, 0.0);
    double all = 0.0;
    for (int s = 0; s < n_seg; ++s) {
      double acc = 0.0;
      for (int64_t i = 0; i < seg_count[s]; ++i) {
        const double u = (double)(grad[seg_off[s] + i] * inv_scale);
        acc = norm_inf ? fmax(acc, fabs(u)) : acc + u * u;
      }
      sums[s] = acc;
      all = norm_inf ? fmax(all, acc) : all + acc;
      const float norm = norm_inf ? (float)acc : sqrtf((float)acc);
      if (norms_out) norms_out[s] = norm;
      coef[s] = sgd_clip_clamp(h.clip_value / sgd_clip_denominator(norm));
    }
    if (h.clip_type == SGD_CLIP_FULL_MODEL) {
      const float norm = norm_inf ? (float)all : sqrtf((float)all);
      const float c = sgd_clip_clamp(h.clip_value / sgd_clip_denominator(norm));
      for (int s = 0; s < n_seg; ++s) coef[s] = c;
    }
    if (coef_out) for (int s = 0; s < n_seg; ++s) coef_out[s] = coef[s];
  }
  if (skip && *skip) return RS_OK;
  for (const SgdChunk& c : chunks) {
    const bool in_seg = c.seg >= 0, bias = in_seg && (c.flags & SGD_SEG_BIAS);
    const float lr_seg = bias ? h.lr_bias : h.lr, wd_seg = bias ? h.wd_bias : h.wd;
    const int by_value = in_seg && h.clip_type == SGD_CLIP_VALUE;
    const float cf = in_seg ? coef[c.seg] : 1.f;
    for (int i = 0; i < c.count; ++i)
      sgd_rule(w + c.off + i, momentum_buf + c.off + i, grad[c.off + i], h.inv_scale, lr_seg, wd_seg, h.momentum, h.nesterov, by_value, h.clip_value, cf);
  }
  return RS_OK;
}

int rs_op_fold_weights(const float* w32, const float* scale, void* w_fwd, void* w_bwd, int cout, int cin, int kh, int kw, int kpad,
                       int kpad_t, void* stream) {
  return launch_fold_weights(w32, scale, (half_t*)w_fwd, (half_t*)w_bwd, cout, cin, kh, kw, kpad, cout, kpad_t, (hipStream_t)stream);
}

}  // extern "C"
