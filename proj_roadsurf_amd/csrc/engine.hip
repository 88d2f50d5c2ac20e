// librs_engine.so host side: C ABI (include/rs_engine.h), weight blob, workspace and the op list
// of one GeneralizedRCNN.inference pass ([EXT d2: modeling/meta_arch/rcnn.py]; topology fixed by
// R:config/detectron2_config_3bands.yaml).  All device work is enqueued on one HIP stream with
// fixed-capacity buffers and device-side counts: no host synchronisation inside a forward.
#include <stdarg.h>
#include <string.h>

#include <cmath>

#include "engine_internal.h"
#include "polygon_pool.h"
#include "train.h"
#include "val_ap.h"
#include "poly_vote.h"

// ------------------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";

// ---------------------------------------------------------------- debug switches: the one place that reads the environment
static RsDebug g_debug;
static bool g_debug_loaded = false;
void rs_debug_reload() {
  RsDebug d;
  auto rd = [](const char* name, int* v) { const char* e = getenv(name); if (e && *e) *v = atoi(e); };
  rd("RS_CONV_SINGLE_STAGE_NK", &d.conv_single_stage_nk); rd("RS_CONV_PERSIST", &d.conv_persist); rd("RS_CONV_TUNED", &d.conv_tuned);
  rd("RS_CONV_DEEP", &d.conv_deep); rd("RS_CONV_WIDE_PX", &d.conv_wide_px); rd("RS_CONV_WREG", &d.conv_wreg); rd("RS_CONV_WIDE1X1", &d.conv_wide1x1); rd("RS_WREG_DBG", &d.wreg_dbg); rd("RS_ROI_BWD_ATOMIC", &d.roi_bwd_atomic); rd("RS_WREG_WAVES", &d.wreg_waves); rd("RS_STEM_SMALL_TILE", &d.stem_small_tile); rd("RS_DEEP_DBG", &d.deep_dbg);
  rd("RS_DECONV_VARIANT", &d.deconv_variant); rd("RS_FUSE_MASK_PREDICTOR", &d.fuse_mask_predictor); rd("RS_SIDE_STREAM", &d.side_stream);
  rd("RS_NARROW_ROIALIGN", &d.narrow_roialign); rd("RS_USE_GLDS", &d.use_glds); rd("RS_FUSE_SHORTCUT", &d.fuse_shortcut); rd("RS_MERGE_LEVELS", &d.merge_levels); rd("RS_FUSE_RPN_HEADS", &d.fuse_rpn_heads); rd("RS_DEEP_TAIL", &d.deep_tail); rd("RS_DEEP_TILE_PX", &d.deep_tile_px); rd("RS_FUSE_BNECK", &d.fuse_bneck); rd("RS_FUSE_STEM", &d.fuse_stem);
  rd("RS_USE_GRAPH", &d.use_graph); rd("RS_GRAPH_SMALL", &d.graph_small); rd("RS_TRAIN_ROI_SIDE", &d.train_roi_side);
  rd("RS_TRAIN_SIDE", &d.train_side); rd("RS_WGRAD_TARGET", &d.wgrad_target); rd("RS_WGRAD_CB", &d.wgrad_cb);
  rd("RS_SELECT_DEBUG", &d.select_debug); rd("RS_NMS_DEBUG", &d.nms_debug); rd("RS_ROI_WINDOW", &d.roi_window); rd("RS_ROI_ORDER", &d.roi_order);
  rd("RS_POLY_EDGE_CAP", &d.poly_edge_cap); rd("RS_POLY_VERTEX_CAP", &d.poly_vertex_cap);
  g_debug = d;
  g_debug_loaded = true;
}
const RsDebug& rs_debug() {
  if (!g_debug_loaded) rs_debug_reload();
  return g_debug;
}
void rs_set_error(const char* fmt, ...) {
  va_list a;
  va_start(a, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, a);
  va_end(a);
}

// host-only helpers -------------------------------------------------------------------------
extern "C" void rs_resize_shape(int h, int w, int short_edge, int max_size, int* new_h, int* new_w) {
  // [EXT d2: data/transforms/augmentation_impl.py ResizeShortestEdge.get_output_shape]
  double scale = (double)short_edge * 1.0 / (double)(h < w ? h : w);
  double newh, neww;
  if (h < w) { newh = short_edge; neww = scale * w; } else { newh = scale * h; neww = short_edge; }
  const double mx = newh > neww ? newh : neww;
  if (mx > max_size) {
    scale = (double)max_size * 1.0 / mx;
    newh = newh * scale;
    neww = neww * scale;
  }
  *new_w = (int)(neww + 0.5);
  *new_h = (int)(newh + 0.5);
}

extern "C" int rs_resize_coeffs(int in_size, int out_size, int32_t* bounds, int32_t* coeffs) {
  // Pillow src/libImaging/Resample.c precompute_coeffs (bilinear, support 1) + normalize_coeffs_8bpc
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (!bounds || !coeffs) return ksize;
  const double ss = 1.0 / filterscale;
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < ksize; ++x) w[x] = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0) a = -a;
      const double v = a < 1.0 ? 1.0 - a : 0.0;
      w[x] = v;
      ww += v;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) w[x] /= ww;
    for (int x = 0; x < ksize; ++x) {
      const double v = w[x] * (double)(1 << 22);
      coeffs[xx * ksize + x] = v < 0 ? (int)(v - 0.5) : (int)(v + 0.5);
    }
    bounds[xx * 2] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
  return ksize;
}

// =================================================================================== engine
int rs_engine::parse_blob(const void* data, size_t nbytes) {
  const uint8_t* b = (const uint8_t*)data;
  RS_CHECK(nbytes >= 16, RS_ERR_BLOB, "weight blob too small");
  uint32_t hdr[4];
  memcpy(hdr, b, 16);
  RS_CHECK(hdr[0] == 0x52534557u && hdr[1] == 1u, RS_ERR_BLOB, "bad weight blob magic/version %08x/%u", hdr[0], hdr[1]);
  const size_t ent = 96 + 4 + 4 + 32 + 8 + 8;
  RS_CHECK(16 + ent * hdr[2] <= nbytes, RS_ERR_BLOB, "weight blob truncated");
  RS_HIP(hipMalloc(&blob_dev, nbytes));
  RS_HIP(hipMemcpy(blob_dev, data, nbytes, hipMemcpyHostToDevice));
  for (uint32_t i = 0; i < hdr[2]; ++i) {
    const uint8_t* e = b + 16 + ent * i;
    char name[97];
    memcpy(name, e, 96);
    name[96] = 0;
    BlobEntry be;
    uint32_t dt, nd;
    uint64_t dims[4], off, nb;
    memcpy(&dt, e + 96, 4);
    memcpy(&nd, e + 100, 4);
    memcpy(dims, e + 104, 32);
    memcpy(&off, e + 136, 8);
    memcpy(&nb, e + 144, 8);
    RS_CHECK(off + nb <= nbytes, RS_ERR_BLOB, "weight blob entry %s out of range", name);
    be.host = b + off;
    be.dev = (char*)blob_dev + off;
    be.dtype = (int)dt;
    be.ndim = (int)nd;
    for (int d = 0; d < 4; ++d) be.dims[d] = (int64_t)dims[d];
    be.nbytes = nb;
    blob[name] = be;
  }
  return RS_OK;
}

// One conv / linear stage (ConvDesc).
int rs_engine::add_conv(const std::string& name, const std::string& wname, const Act& in, const Act& out, const ConvDesc& d) {
  const int k = d.k, stride = d.stride, pad = d.pad, stride2 = d.stride2, units_per_tile = d.units_per_tile;
  const int cin_real = d.cin_real ? d.cin_real : in.C;
  const Act *res = d.res, *up = d.up, *in2 = d.in2;
  const BlobEntry* w = findw(wname);
  const BlobEntry* b = find(wname + ".b");
  RS_CHECK(w && b, RS_ERR_BLOB, "weights for %s missing from blob", wname.c_str());
  RS_CHECK(w->dtype == (f32 ? DT_F32 : DT_F16) && b->dtype == DT_F32, RS_ERR_BLOB, "weights for %s have wrong dtype", wname.c_str());
  ConvParams p;
  memset(&p, 0, sizeof p);
  { int rc = set_split(&p, wname, w, &in, &out, res, up, in2); if (rc) return rc; }
  p.in = in.p; p.w = (const half_t*)w->dev; p.bias = (const float*)b->dev; p.out = out.p;
  p.res = res ? res->p : nullptr;
  p.up = up ? up->p : nullptr;
  p.Ho = out.H; p.Wo = out.W;
  p.in_Hp = in.Hp(); p.in_Wp = in.Wp(); p.in_Cs = in.C; p.in_off = in.pad - pad;
  p.stride = stride; p.KH = k; p.KW = k; p.Cin = in.C;
  p.Kpad = (int)w->dims[1];
  p.Cout = out.C;
  p.out_Hp = out.Hp(); p.out_Wp = out.Wp(); p.out_Cs = out.C; p.out_pad = out.pad;
  if (up) { p.up_Hp = up->Hp(); p.up_Wp = up->Wp(); p.up_Cs = up->C; p.up_pad = up->pad; }
  p.relu = d.relu ? 1 : 0;
  if (in2) {   // second K source: 1x1 taps at stride2 (projection shortcut folded into conv3)
    RS_CHECK((out.H - 1) * stride2 < in2->H && (out.W - 1) * stride2 < in2->W && in2->C % 64 == 0, RS_ERR_ARG, "%s: second source geometry", name.c_str());
    p.in2 = in2->p; p.in2_Hp = in2->Hp(); p.in2_Wp = in2->Wp(); p.in2_Cs = in2->C; p.in2_off = in2->pad;
    p.stride2 = stride2; p.Cin2 = in2->C;
  }
  RS_CHECK(in.pad >= pad, RS_ERR_ARG, "%s: input halo %d < conv pad %d", name.c_str(), in.pad, pad);
  RS_CHECK(wrows(w) >= out.C, RS_ERR_BLOB, "%s: weight rows %d < Cout %d", name.c_str(), wrows(w), out.C);
  RS_CHECK((out.H - 1) * stride + k - 2 * pad <= in.H + (stride - 1), RS_ERR_ARG, "%s: geometry", name.c_str());
  if (res) RS_CHECK(res->H == out.H && res->W == out.W && res->C == out.C && res->pad == out.pad, RS_ERR_ARG, "%s: residual geometry", name.c_str());
  if (in.C < 64) {
    // small-Cin (stem) path: per-16-byte-chunk element offsets.  C == 8: one tap per chunk.  C == 4: the tap row
    // is padded to 8 taps (the 8th has zero weights) and a chunk holds two horizontally adjacent taps, so
    // K = kh*8*4 = 224 -> 256 instead of 49*8 = 392 -> 448.
    RS_CHECK(in.C == 8 || in.C == 4, RS_ERR_UNSUPPORTED, "%s: Cin %d", name.c_str(), in.C);
    std::vector<int> koff(p.Kpad / 8, 0);
    if (in.C == 8) {
      for (int t = 0; t < k * k && t < (int)koff.size(); ++t) koff[t] = ((t / k) * p.in_Wp + (t % k)) * in.C;
    } else {
      RS_CHECK(k == 7 && (p.in_Wp & 1) == 0 && ((in.pad - pad) & 1) == 0 && stride == 2, RS_ERR_UNSUPPORTED, "%s: C=4 stem needs 7x7 s2 and even pitch", name.c_str());
      p.KW = 8;
      for (int t = 0; t < k * 4 && t < (int)koff.size(); ++t) koff[t] = ((t / 4) * p.in_Wp + (t % 4) * 2) * in.C;
    }
    int* dk = nullptr;
    int rc = alloc((void**)&dk, koff.size() * 4);
    if (rc) return rc;
    RS_HIP(hipMemcpyAsync(dk, koff.data(), koff.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipStreamSynchronize(stream));
    p.koff = dk;
  }
  const int m_per_image = out.H * out.W * units_per_tile;
  p.m_count = d.m_count;
  p.m_mul = out.H * out.W;
  const double flops = 2.0 * m_per_image * ((double)k * k * cin_real + (in2 ? in2->C : 0)) * out.C;
  // algorithmic bytes: the input pixels the convolution actually reads (a stride-s 1x1 touches every s-th pixel of every
  // s-th row only), the output once, the residual once, the second K source at the output's pixel count
  const double in_px = k >= stride ? (double)in.H * in.W : (double)out.H * out.W * k * k;
  const double bytes = 2.0 * planes() * (in_px * in.C * units_per_tile + (double)m_per_image * out.C * (1 + (res ? 1 : 0)) +
                                        (in2 ? (double)m_per_image * in2->C : 0.0));
  if (d.defer) {
    d.defer->p = p; d.defer->m_per_image = m_per_image; d.defer->flops = flops; d.defer->bytes = bytes;
    return RS_OK;
  }
  Stage& st = add_stage(name, flops, bytes, &p.sat);   // before the lambda copies p
  st.fn = conv_stage_fn(p, m_per_image, -1, use_glds);
  return RS_OK;
}

// The launch of a conv / linear stage.  Everywhere but in the forward engine of an fp32 trainer this is launch_conv(p, s, variant, glds)
// and nothing else.  There, a stage whose shape the split forward serves also reads fwd_mode when it runs (engine_internal.h).
std::function<int(int, hipStream_t)> rs_engine::conv_stage_fn(const ConvParams& p_in, int m_per_image, int variant, int glds) {
  ConvParams p = p_in;
  int li = -1;
  if (fwd_split_capable && p.mode == 0 && !p.in2 && !p.koff && p.in_Cs == p.Cin && p.Kpad % 64 == 0 && p.in_off >= 0 &&
      conv_fwd_split_serves(p.Cout, p.Cin, p.KH, p.KW, p.stride)) {
    for (size_t i = 0; i < fws_layers.size(); ++i)
      if (fws_layers[i].w == (const float*)p.w && fws_layers[i].rows == p.Cout && fws_layers[i].kpad == p.Kpad) li = (int)i;
    if (li < 0) {
      FwdSplitLayer L;
      L.w = (const float*)p.w; L.rows = p.Cout; L.kpad = p.Kpad;
      li = (int)fws_layers.size();
      fws_layers.push_back(L);
    }
    ConvParams full = p;
    full.M = max_batch * m_per_image;
    full.m_count = nullptr;
    const long long el = fwd_split_x_elems(full);
    if (el > fws_cap) fws_cap = el;
  }
  if (li < 0) return [p, m_per_image, variant, glds](int n, hipStream_t s) mutable { p.M = n * m_per_image; return launch_conv(p, s, variant, glds); };
  rs_engine* self = this;
  return [p, m_per_image, variant, glds, li, self](int n, hipStream_t s) mutable {
    p.M = n * m_per_image;
    if (self->fwd_mode != 1) return launch_conv(p, s, variant, glds);
    const FwdSplitLayer& L = self->fws_layers[li];
    ConvParams q = p;                          // q.in: the fp32 X
    int rc = launch_fwd_split_planes(q, self->fws_scratch, self->fws_cap, s);
    if (rc) return rc;
    q.split = 1; q.x_amax = (const unsigned*)self->fws_scratch;
    q.in = (const half_t*)((const char*)self->fws_scratch + WGS_HEAD_BYTES); q.in_lo = self->fws_cap;
    q.w = L.planes; q.w_lo = (long long)L.rows * L.kpad; q.wscale = L.inv;
    return launch_conv(q, s, -1, 1);           // the split rule picks the tile (a forced fp32 variant does not carry over)
  };
}

int rs_engine::fwd_split_weights(bool folded_only) {
  RS_CHECK(fws_table && fws_n_all > 0, RS_ERR_ARG, "engine: the split forward mode has no weight planes");
  if (folded_only) return fws_n_fold > 0 ? launch_split_rows_table(fws_table + fws_n_all, fws_n_fold, fws_rows_fold, stream) : RS_OK;
  return launch_split_rows_table(fws_table, fws_n_all, fws_rows_all, stream);
}

int rs_engine::fwd_split_enable(const std::set<const void*>& folded) {
  RS_CHECK(fwd_split_capable && !fws_layers.empty(), RS_ERR_UNSUPPORTED, "engine: only the forward engine of an fp32 trainer carries the split forward mode");
  std::vector<SplitRowsDesc> tab;
  for (FwdSplitLayer& L : fws_layers) {
    if (L.planes) continue;
    int rc = alloc((void**)&L.planes, (size_t)L.rows * L.kpad * 4);
    if (!rc) rc = alloc((void**)&L.inv, (size_t)L.rows * 4);
    if (rc) return rc;
  }
  unsigned rows = 0;
  for (const FwdSplitLayer& L : fws_layers) {
    tab.push_back(SplitRowsDesc{L.w, L.planes, L.inv, L.rows, L.kpad, rows});
    rows += (unsigned)L.rows;
  }
  const int n_all = (int)tab.size();
  unsigned rows_fold = 0;
  for (const FwdSplitLayer& L : fws_layers) {
    if (!folded.count((const void*)L.w)) continue;
    tab.push_back(SplitRowsDesc{L.w, L.planes, L.inv, L.rows, L.kpad, rows_fold});
    rows_fold += (unsigned)L.rows;
  }
  if (!fws_table) { int rc = alloc((void**)&fws_table, 2 * fws_layers.size() * sizeof(SplitRowsDesc)); if (rc) return rc; }
  RS_HIP(hipMemcpyAsync(fws_table, tab.data(), tab.size() * sizeof(SplitRowsDesc), hipMemcpyHostToDevice, stream));
  RS_HIP(hipStreamSynchronize(stream));      // tab is a local
  fws_n_all = n_all; fws_n_fold = (int)tab.size() - n_all; fws_rows_all = rows; fws_rows_fold = rows_fold;
  return alloc(&fws_scratch, dgrad_split_scratch_bytes(fws_cap));
}

// 0 = fp32 matrix cores, 1 = split operands.  Every switch to 1 splits every layer's current weight; a captured forward is dropped.
int rs_engine::set_fwd_mode(int mode, const std::set<const void*>& folded) {
  if (mode == 1 && !fws_scratch) { int rc = fwd_split_enable(folded); if (rc) return rc; }
  if (mode == 1) { int rc = fwd_split_weights(false); if (rc) return rc; }
  if (mode != fwd_mode) {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second);
    graphs.clear();
  }
  fwd_mode = mode;
  return RS_OK;
}

// One stage = one conv_deep launch over several maps (launch_conv_deep_multi)
int rs_engine::add_merged_convs(const std::string& name, const std::vector<DeferredConv>& d) {
  RS_CHECK(!d.empty() && d.size() <= RS_MAX_SEGS, RS_ERR_ARG, "%s: %d maps", name.c_str(), (int)d.size());
  ConvParams common = d[0].p;
  std::vector<ConvSeg> segs(d.size());
  std::vector<int> mpi(d.size());
  double flops = 0, bytes = 0;
  for (size_t i = 0; i < d.size(); ++i) {
    const ConvParams& q = d[i].p;
    RS_CHECK(q.Cin == common.Cin && q.Cout == common.Cout && q.KH == common.KH && q.KW == common.KW && q.stride == 1 && q.in_Cs == common.in_Cs &&
                 q.in_off == common.in_off && q.out_Cs == common.out_Cs && q.out_pad == common.out_pad && q.Kpad == common.Kpad && q.relu == common.relu &&
                 !q.res && !q.up && !q.in2 && !q.m_count && q.mode == 0 && !q.out_f32,
             RS_ERR_ARG, "%s: map %d does not share the launch parameters of map 0", name.c_str(), (int)i);
    RS_CHECK(q.head_w == common.head_w && q.head_b == common.head_b && q.head_scale == common.head_scale, RS_ERR_ARG, "%s: map %d has another fused head", name.c_str(), (int)i);
    RS_CHECK(q.split == common.split && q.w_lo == common.w_lo, RS_ERR_ARG, "%s: map %d differs in the split-operand fields", name.c_str(), (int)i);
    segs[i].in = q.in; segs[i].w = q.w; segs[i].bias = q.bias; segs[i].out = q.out; segs[i].head_out = q.head_out;
    segs[i].in_lo = q.in_lo; segs[i].out_lo = q.out_lo; segs[i].wscale = q.wscale;
    segs[i].Ho = q.Ho; segs[i].Wo = q.Wo; segs[i].in_Hp = q.in_Hp; segs[i].in_Wp = q.in_Wp; segs[i].out_Hp = q.out_Hp; segs[i].out_Wp = q.out_Wp;
    mpi[i] = d[i].m_per_image;
    flops += d[i].flops;
    bytes += d[i].bytes;
  }
  Stage& st = add_stage(name, flops, bytes, &common.sat);
  st.fn = [common, segs, mpi](int n, hipStream_t s) {
    g_last_conv_variant = 12;
    return launch_conv_deep_multi(common, segs.data(), mpi.data(), (int)segs.size(), n, s);
  };
  return RS_OK;
}

int rs_engine::resize_tab(int in_size, int out_size, std::map<int, ResizeTab>& cache, ResizeTab* out) {
  auto it = cache.find(out_size);
  if (it == cache.end()) {
    ResizeTab t;
    t.ks = rs_resize_coeffs(in_size, out_size, nullptr, nullptr);
    std::vector<int32_t> b((size_t)out_size * 2), k((size_t)out_size * t.ks);
    rs_resize_coeffs(in_size, out_size, b.data(), k.data());
    int rc;
    if ((rc = alloc((void**)&t.b, b.size() * 4))) return rc;
    if ((rc = alloc((void**)&t.k, k.size() * 4))) return rc;
    RS_HIP(hipMemcpyAsync(t.b, b.data(), b.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipMemcpyAsync(t.k, k.data(), k.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipStreamSynchronize(stream));          // the host vectors go out of scope
    it = cache.emplace(out_size, t).first;
  }
  *out = it->second;
  return RS_OK;
}

// n = 0: every image fills the canvas again
int rs_engine::set_image_sizes(const int32_t* new_h, const int32_t* new_w, int n) {
  RS_CHECK(n >= 0 && n <= max_batch, RS_ERR_ARG, "set_image_sizes: %d images, engine built for %d", n, max_batch);
  std::vector<float> hw((size_t)max_batch * 2);
  for (int i = 0; i < max_batch; ++i) { hw[2 * i] = (float)net_h; hw[2 * i + 1] = (float)net_w; }
  for (int i = 0; i < n; ++i) {
    RS_CHECK(new_h[i] >= 1 && new_h[i] <= net_h && new_w[i] >= 1 && new_w[i] <= net_w, RS_ERR_ARG,
             "image %d: %d x %d does not fit the %d x %d canvas", i, new_h[i], new_w[i], net_h, net_w);
    hw[2 * i] = (float)new_h[i]; hw[2 * i + 1] = (float)new_w[i];
  }
  for (int i = 0; i < n; ++i) {                     // build the tables now: the stage itself must not synchronise
    ResizeTab t;
    int rc;
    if ((rc = resize_tab(tile_w, new_w[i], tab_h, &t))) return rc;
    if ((rc = resize_tab(tile_h, new_h[i], tab_v, &t))) return rc;
  }
  img_new_h.assign(new_h, new_h + n);
  img_new_w.assign(new_w, new_w + n);
  RS_HIP(hipMemcpyAsync(img_hw_dev, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, stream));
  RS_HIP(hipStreamSynchronize(stream));
  return RS_OK;
}

static const std::string kBottomUp = "backbone.bottom_up.";

int rs_engine::build() {
  const rs_spec& S = spec;
  rs_resize_shape(tile_h, tile_w, S.min_size_test, S.max_size_test, &net_h, &net_w);
  const int dv = S.size_divisibility;
  pad_h = (net_h + dv - 1) / dv * dv;
  pad_w = (net_w + dv - 1) / dv * dv;
  RS_CHECK(S.fpn_out_channels == 256 && S.mask_conv_dim == 256, RS_ERR_UNSUPPORTED, "FPN/mask width must be 256");
  RS_CHECK(S.num_levels == 5, RS_ERR_UNSUPPORTED, "RPN must use p2..p6");
  RS_CHECK(S.rpn_pre_nms_topk <= 1024 && S.rpn_post_nms_topk <= 1024, RS_ERR_UNSUPPORTED, "RPN top-k > 1024");
  RS_CHECK(S.num_classes >= 1 && S.num_classes <= RS_MAX_CLASSES, RS_ERR_UNSUPPORTED, "NUM_CLASSES %d outside [1,%d]", S.num_classes, RS_MAX_CLASSES);
  // the many-class merge is checked here, with both numbers in the message; up to RS_DET_GROUP classes the launcher's own check stands as before
  if (S.num_classes > RS_DET_GROUP) { const int rc0 = det_merge_check(S.num_classes, S.detections_per_image); if (rc0) return rc0; }
  RS_CHECK(S.in_channels >= 1 && S.in_channels <= 4 && S.in_channels == tile_c, RS_ERR_ARG, "tile channels %d vs PIXEL_MEAN %d", tile_c, S.in_channels);
  RS_CHECK(!S.mask_on || S.mask_pooler_resolution * 2 == RS_MASK_SIDE, RS_ERR_UNSUPPORTED, "mask side must be 28");
  int rc;
  if (!frozen_fusions_only) {
    if ((rc = alloc((void**)&sat_dev, kSatCap * 8))) return rc;
    if ((rc = alloc((void**)&sat_snap, kSatCap * 8))) return rc;
    RS_HIP(hipHostMalloc((void**)&h_sat_copy, kSatCap * 8, hipHostMallocDefault));
  }
  Graph g;
  if ((rc = build_input(g))) return rc;
  if ((rc = build_stem(g))) return rc;
  if ((rc = build_res_stages(g))) return rc;
  if ((rc = build_fpn(g))) return rc;
  if ((rc = build_rpn(g))) return rc;
  if ((rc = build_box_head(g))) return rc;
  if (S.mask_on && (rc = build_mask_head(g))) return rc;
  RS_CHECK(stages.size() <= (size_t)kSatCap, RS_ERR_UNSUPPORTED, "%d stages: more than the %d saturation counters", (int)stages.size(), kSatCap);
  h_sat.assign(stages.size(), 0);
  RS_HIP(hipStreamSynchronize(stream));
  return RS_OK;
}

// ---- resize tables + input staging + preprocess
int rs_engine::build_input(Graph& g) {
  const rs_spec& S = spec;
  const int NB = max_batch;
  int rc;
  if ((rc = new_tensor(&tiles_dev, "tiles", DT_U8, {NB, tile_h, tile_w, tile_c}))) return rc;
  PreprocParams pp;
  memset(&pp, 0, sizeof pp);
  pp.need_h = net_w != tile_w;
  pp.need_v = net_h != tile_h;
  {
    const int ksh = rs_resize_coeffs(tile_w, net_w, nullptr, nullptr);
    const int ksv = rs_resize_coeffs(tile_h, net_h, nullptr, nullptr);
    std::vector<int32_t> hb(net_w * 2), hk((size_t)net_w * ksh), vb(net_h * 2), vk((size_t)net_h * ksv);
    rs_resize_coeffs(tile_w, net_w, hb.data(), hk.data());
    rs_resize_coeffs(tile_h, net_h, vb.data(), vk.data());
    int *dhb, *dhk, *dvb, *dvk;
    if ((rc = alloc((void**)&dhb, hb.size() * 4))) return rc;
    if ((rc = alloc((void**)&dhk, hk.size() * 4))) return rc;
    if ((rc = alloc((void**)&dvb, vb.size() * 4))) return rc;
    if ((rc = alloc((void**)&dvk, vk.size() * 4))) return rc;
    RS_HIP(hipMemcpyAsync(dhb, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipMemcpyAsync(dhk, hk.data(), hk.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipMemcpyAsync(dvb, vb.data(), vb.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipMemcpyAsync(dvk, vk.data(), vk.size() * 4, hipMemcpyHostToDevice, stream));
    RS_HIP(hipStreamSynchronize(stream));
    pp.hb = dhb; pp.hk = dhk; pp.vb = dvb; pp.vk = dvk; pp.ksh = ksh; pp.ksv = ksv;
  }
  Act& x0 = g.x0;
  if ((rc = new_act(&x0, "net_input", NB, pad_h, pad_w, 4, 3))) return rc;
  pp.out = x0.p; pp.H = tile_h; pp.W = tile_w; pp.C = tile_c; pp.new_h = net_h; pp.new_w = net_w;
  pp.out_Hp = x0.Hp(); pp.out_Wp = x0.Wp(); pp.flip = S.flip_channels; pp.out_f32 = prec_code();
  pp.out_lo = x0.lo;
  for (int c = 0; c < 4; ++c) { pp.mean[c] = S.pixel_mean[c]; pp.stdv[c] = S.pixel_std[c] == 0.f ? 1.f : S.pixel_std[c]; }
  pp.tiles = tiles_dev;
  Stage& st = add_stage("preprocess", 0, (double)tile_h * tile_w * tile_c + (double)net_h * net_w * 8, &pp.sat);
  const size_t x0_bytes = (size_t)NB * x0.Hp() * x0.Wp() * 4 * esize();       // one plane
  const int planes = this->planes();
  st.fn = [this, pp, x0_bytes, planes](int n, hipStream_t s) mutable {
    if (img_new_h.empty()) {
      pp.N = n;
      return launch_preprocess(pp, s);
    }
    // images of different sizes in one canvas: zeros (the padding value of ImageList.from_tensors) outside each image
    RS_CHECK((int)img_new_h.size() >= n, RS_ERR_ARG, "per-image sizes set for %d images, batch of %d", (int)img_new_h.size(), n);
    RS_HIP(hipMemsetAsync((void*)pp.out, 0, x0_bytes * planes, s));
    for (int i = 0; i < n; ++i) {
      PreprocParams q = pp;
      ResizeTab th, tv;
      int rc;
      if ((rc = resize_tab(tile_w, img_new_w[i], tab_h, &th))) return rc;
      if ((rc = resize_tab(tile_h, img_new_h[i], tab_v, &tv))) return rc;
      q.N = 1;
      q.tiles = pp.tiles + (size_t)i * tile_h * tile_w * tile_c;
      q.out = (half_t*)((char*)pp.out + (size_t)i * (x0_bytes / max_batch));
      q.new_h = img_new_h[i]; q.new_w = img_new_w[i];
      q.need_h = q.new_w != tile_w; q.need_v = q.new_h != tile_h;
      q.hb = th.b; q.hk = th.k; q.ksh = th.ks; q.vb = tv.b; q.vk = tv.k; q.ksv = tv.ks;
      if ((rc = launch_preprocess(q, s))) return rc;
    }
    return RS_OK;
  };
  if ((rc = alloc((void**)&img_hw_dev, (size_t)NB * 8))) return rc;
  return set_image_sizes(nullptr, nullptr, 0);
}

// ---- stem: conv 7x7 s2 + FrozenBN + ReLU, max-pool 3x3 s2
int rs_engine::build_stem(Graph& g) {
  const rs_spec& S = spec;
  const std::string& bu = kBottomUp;
  const Act& x0 = g.x0;
  const int h2 = pad_h / 2, w2 = pad_w / 2, h4 = pad_h / 4, w4 = pad_w / 4;
  Act stem;
  Act& c1 = g.c1;
  int rc;
  if ((rc = new_act(&stem, "stem_conv", max_batch, h2, w2, S.stem_out_channels, 1))) return rc;
  if ((rc = new_act(&c1, "stem", max_batch, h4, w4, S.stem_out_channels, 1))) return rc;
  const BlobEntry* stem_w = findw(bu + "stem.conv1f");          // fragment-ordered copy of the 64 x 256 stem matrix
  const BlobEntry* stem_b = find(bu + "stem.conv1.b");
  const BlobEntry* stem_si = split ? find(bu + "stem.conv1.wsi") : nullptr;
  const bool stem_frozen = !frozen_fusions_only || freeze_at >= 1;    // a trainer that differentiates the stem keeps stem_conv
  if (fuse_stem && stem_frozen && !f32 && use_glds > 0 && S.stem_out_channels == 64 && x0.C == 4 && x0.pad == 3 && stem_w && stem_b && (!split || stem_si) &&
      (long long)stem_w->dims[0] * stem_w->dims[1] == planes() * 7 * 4 * 64 * 8 && (pad_h & 3) == 0 && (pad_w & 3) == 0) {
    // conv 7x7 s2 + FrozenBN + ReLU + max-pool 3x3 s2 in one launch (stem_fused.hip): the 400 x 400 x 64 map never reaches HBM
    const double flops = 2.0 * h2 * w2 * 49.0 * S.in_channels * 64;
    const double bytes = 2.0 * planes() * ((double)pad_h * pad_w * 4 + (double)h4 * w4 * 64);
    if (!split) {
      StemPoolParams sp;
      memset(&sp, 0, sizeof sp);
      sp.in = x0.p; sp.wf = (const half_t*)stem_w->dev; sp.bias = (const float*)stem_b->dev; sp.out = c1.p;
      sp.in_Hp = x0.Hp(); sp.in_Wp = x0.Wp();
      sp.Hc = h2; sp.Wc = w2; sp.Hq = h4; sp.Wq = w4;
      Stage& st = add_stage("stem.conv1+maxpool", flops, bytes, &sp.sat);
      st.fn = [sp](int n, hipStream_t s) mutable { sp.N = n; g_last_conv_variant = 21; return launch_stem_pool(sp, s); };
    } else {
      // the same launch on hi + lo planes (stem_fused.hip stem_pool_split_kernel): bit-identical to the stand-alone split stem + split max-pool
      StemPoolSplitParams sp;
      memset(&sp, 0, sizeof sp);
      sp.in = x0.p; sp.in_lo = x0.lo; sp.wf = (const half_t*)stem_w->dev; sp.wscale = (const float*)stem_si->dev;
      sp.bias = (const float*)stem_b->dev; sp.out = c1.p; sp.out_lo = c1.lo;
      sp.in_Hp = x0.Hp(); sp.in_Wp = x0.Wp();
      sp.Hc = h2; sp.Wc = w2; sp.Hq = h4; sp.Wq = w4;
      Stage& st = add_stage("stem.conv1+maxpool", flops, bytes, &sp.sat);
      st.fn = [sp](int n, hipStream_t s) mutable { sp.N = n; g_last_conv_variant = 21; return launch_stem_pool_split(sp, s); };
    }
    return RS_OK;
  }
  ConvDesc d{7, 2, 3, true};
  d.cin_real = S.in_channels;
  if ((rc = add_conv("stem.conv1", bu + "stem.conv1", x0, stem, d))) return rc;
  const bool f = f32, sp = split;
  add_stage("stem.maxpool", 0, 2.0 * ((double)h2 * w2 + (double)h4 * w4) * S.stem_out_channels).fn = [stem, c1, f, sp](int n, hipStream_t s) {
    if (sp) return launch_maxpool_split(stem.p, stem.lo, c1.p, c1.lo, n, stem.H, stem.W, c1.H, c1.W, c1.C, s);
    return f ? launch_maxpool_f32((const float*)stem.p, (float*)c1.p, n, stem.H, stem.W, c1.H, c1.W, c1.C, s)
             : launch_maxpool(stem.p, c1.p, n, stem.H, stem.W, c1.H, c1.W, c1.C, s);
  };
  return RS_OK;
}

// ---- res2..res5
int rs_engine::build_res_stages(Graph& g) {
  ResCursor r;
  r.cur = g.c1;
  r.cout = spec.res2_out_channels;
  for (int si = 0; si < 4; ++si) {
    for (int bi = 0; bi < spec.res_blocks[si]; ++bi) {
      int rc = build_bottleneck(r, si, bi);
      if (rc) return rc;
    }
    g.res_out[si] = r.cur;
    r.bott *= 2;
    r.cout *= 2;
  }
  return RS_OK;
}

// One bottleneck block: conv1 1x1, conv2 3x3, conv3 1x1 + shortcut + ReLU, with whatever of it this engine fuses
int rs_engine::build_bottleneck(ResCursor& r, int si, int bi) {
  const rs_spec& S = spec;
  const std::string& bu = kBottomUp;
  const int NB = max_batch, bott = r.bott, cout = r.cout;
  const Act cur = r.cur;
  const std::string stage = "res" + std::to_string(si + 2);
  const std::string nm = stage + "." + std::to_string(bi), next = stage + "." + std::to_string(bi + 1);
  const std::string wn = bu + nm;
  const int stride = (bi == 0 && si > 0) ? 2 : 1;
  const int s1 = S.stride_in_1x1 ? stride : 1, s3 = S.stride_in_1x1 ? 1 : stride;
  const int oh = cur.H / stride, ow = cur.W / stride;
  int rc;
  Act t1, t2, sc, out;
  // Fused tail (bneck_fused.hip): identity-shortcut blocks of the 64- and 128-wide stages run conv2 + conv3 (+ the next block's conv1)
  // in one launch -- t2 is never materialised and the next conv1 reads `out` from registers.  Inference engines, fp16 and split-operand
  // mode (bneck_split.hip: the same chain on hi + lo planes, on the deep-K loop with LDS-DMA staging).
  // Block 0 of the stage has a projection shortcut from the 64-channel stem output at the same resolution: the tail then adds
  // Wsc . x0 as two more K steps instead of the identity residual (needs the folded conv3sc bias = conv3's + the shortcut's; the split
  // mode takes conv3 | shortcut as one [256][128] operand, conv3scp).
  const bool may_fuse = !frozen_fusions_only || (si == 0 && freeze_at >= 2);   // a trainer fuses only inside the frozen res2
  const bool fuse_bneck = this->fuse_bneck && may_fuse, fuse_shortcut = this->fuse_shortcut && may_fuse;
  const bool can_tail = !f32 && fuse_bneck && stride == 1 && (!split || (rs_debug().conv_deep && use_glds > 0));
  const bool tail_proj = can_tail && fuse_shortcut && bi == 0 && bott == 64 && cout == 256 && cur.C == 64 && find(wn + ".conv3sc.b") != nullptr &&
                         (split ? findw(wn + ".conv3scp") != nullptr && find(wn + ".conv3scp.wsi") != nullptr
                                : findw(wn + ".conv3p") != nullptr && findw(wn + ".shortcut") != nullptr);
  const bool tail_id = can_tail && bi > 0 && (bott == 64 || bott == 128) && cout == 4 * bott && findw(wn + ".conv3p") != nullptr &&
                       (!split || find(wn + ".conv3p.wsi") != nullptr);
  const bool tail = tail_proj || tail_id;
  const bool tail_next = tail && bi + 1 < S.res_blocks[si] && findw(bu + next + ".conv1p") != nullptr;
  if (r.have_t1) t1 = r.t1_pre;
  else if ((rc = new_act(&t1, nm + ".conv1", NB, cur.H / s1, cur.W / s1, bott, 1))) return rc;
  if (!tail) { if ((rc = new_act(&t2, nm + ".conv2", NB, oh, ow, bott, 1))) return rc; }
  if ((rc = new_act(&out, bi == S.res_blocks[si] - 1 ? stage : nm + ".out", NB, oh, ow, cout, 1))) return rc;
  const Act* resid = &cur;
  // Projection shortcut: in the fp16 path it is folded into conv3 as a second K source (one GEMM over
  // [conv2 out ; block input], no shortcut tensor written or re-read); the fp32 validation path and
  // RS_FUSE_SHORTCUT=0 keep the reference's two-convolution form.
  const bool proj = cur.C != cout;
  const bool fuse_sc = proj && !tail_proj && !f32 && fuse_shortcut && s3 == 1 && cur.C % 64 == 0 && findw(wn + ".conv3sc") != nullptr;
  if (proj && !fuse_sc && !tail_proj) {
    if ((rc = new_act(&sc, nm + ".shortcut", NB, oh, ow, cout, 1))) return rc;
    if ((rc = add_conv(nm + ".shortcut", wn + ".shortcut", cur, sc, ConvDesc{1, stride, 0, false}))) return rc;
    resid = &sc;
  }
  if (!r.have_t1) { if ((rc = add_conv(nm + ".conv1", wn + ".conv1", cur, t1, ConvDesc{1, s1, 0, true}))) return rc; }
  r.have_t1 = false;
  if (tail) {
    if (tail_next) { if ((rc = new_act(&r.t1_pre, next + ".conv1", NB, oh, ow, bott, 1))) return rc; }
    if ((rc = add_fused_tail(nm, next, t1, cur, out, tail_next ? &r.t1_pre : nullptr, tail_proj))) return rc;
    r.have_t1 = tail_next;
  } else {
    if ((rc = add_conv(nm + ".conv2", wn + ".conv2", t1, t2, ConvDesc{3, s3, 1, true}))) return rc;
    ConvDesc d3{1, 1, 0, true};
    if (fuse_sc) { d3.in2 = &cur; d3.stride2 = stride; } else { d3.res = resid; }
    if ((rc = add_conv(nm + ".conv3", wn + (fuse_sc ? ".conv3sc" : ".conv3"), t2, out, d3))) return rc;
  }
  r.cur = out;
  return RS_OK;
}

// The fused tail of block `nm`: conv2 + conv3 + shortcut (+ conv1 of block `next` into *t1n) in one launch.  `x` is the block input:
// the identity residual, or with `proj` the 64-channel source of res2.0's projection shortcut.
int rs_engine::add_fused_tail(const std::string& nm, const std::string& next, const Act& t1, const Act& x, const Act& out, const Act* t1n, bool proj) {
  const std::string wn = kBottomUp + nm, wnn = kBottomUp + next;
  const char* kind = split ? "fused split tail" : "fused tail";
  const int bott = t1.C, cout = out.C, oh = out.H, ow = out.W;
  const std::string w3n = wn + (proj && split ? ".conv3scp" : ".conv3p");
  const int k3 = proj && split ? bott + 64 : bott;               // K of the conv3 operand
  const BlobEntry *w2 = findw(wn + ".conv2"), *b2 = find(wn + ".conv2.b"), *w3 = findw(w3n), *b3 = find(wn + (proj ? ".conv3sc.b" : ".conv3.b"));
  const BlobEntry *w1 = t1n ? findw(wnn + ".conv1p") : nullptr, *b1 = t1n ? find(wnn + ".conv1.b") : nullptr;
  // split-operand mode: the inverse row scales of the three operands
  const BlobEntry *s2 = split ? find(wn + ".conv2.wsi") : nullptr, *s3 = split ? find(w3n + ".wsi") : nullptr,
                  *s1 = split && t1n ? find(wnn + ".conv1p.wsi") : nullptr;
  RS_CHECK(w2 && b2 && w3 && b3 && (!t1n || (w1 && b1)) && (!split || (s2 && s3 && (!t1n || s1))), RS_ERR_BLOB, "weights of the %s of %s missing", kind, nm.c_str());
  RS_CHECK(wrows(w2) == bott && w2->dims[1] == 9 * bott && wrows(w3) == cout && w3->dims[1] == k3 && (!w1 || (wrows(w1) == bott && w1->dims[1] == cout)),
           RS_ERR_BLOB, "%s of %s: weight shapes", kind, nm.c_str());
  RS_CHECK(t1.pad == 1 && x.pad == 1 && out.pad == 1 && t1.H == oh && x.H == oh && t1.C == bott && x.C == (proj ? 64 : cout), RS_ERR_ARG, "%s of %s: geometry", kind, nm.c_str());
  const int mpi = oh * ow;
  const std::string name = nm + (t1n ? ".conv2+conv3+next.conv1" : ".conv2+conv3");
  const double flops = 2.0 * mpi * (9.0 * bott * bott + (double)(bott + (proj ? 64 : 0)) * cout + (t1n ? (double)cout * bott : 0.0));
  const double bytes = 2.0 * planes() * mpi * ((double)bott + (proj ? 64.0 : (double)cout) + cout + (t1n ? (double)bott : 0.0));   // t1 + x in, out (+ t1n) out
  if (!split) {
    BneckParams bp;
    memset(&bp, 0, sizeof bp);
    bp.t1 = t1.p; bp.w2 = (const half_t*)w2->dev; bp.b2 = (const float*)b2->dev; bp.w3p = (const half_t*)w3->dev; bp.b3 = (const float*)b3->dev;
    bp.out = out.p;
    if (proj) {
      const BlobEntry* wsc = findw(wn + ".shortcut");
      RS_CHECK(wsc && wsc->dims[0] == 256 && wsc->dims[1] == 64, RS_ERR_BLOB, "fused tail of %s: shortcut weight shape", nm.c_str());
      bp.x0 = x.p; bp.wsc = (const half_t*)wsc->dev;
    } else {
      bp.x = x.p;
    }
    if (t1n) { bp.w1p = (const half_t*)w1->dev; bp.b1 = (const float*)b1->dev; bp.t1n = t1n->p; }
    bp.H = oh; bp.W = ow; bp.Hp = out.Hp(); bp.Wp = out.Wp(); bp.CB = bott / 64;
    Stage& st = add_stage(name, flops, bytes, &bp.sat);
    st.fn = [bp, mpi](int n, hipStream_t s) mutable { bp.M = n * mpi; g_last_conv_variant = 13; return launch_bneck_tail(bp, s); };
  } else {
    BneckSplitParams bp;
    memset(&bp, 0, sizeof bp);
    bp.t1 = t1.p; bp.t1_lo = t1.lo;
    bp.w2 = (const half_t*)w2->dev; bp.w2_lo = (long long)bott * 9 * bott; bp.b2 = (const float*)b2->dev; bp.s2 = (const float*)s2->dev;
    bp.w3p = (const half_t*)w3->dev; bp.w3_lo = (long long)cout * k3; bp.b3 = (const float*)b3->dev; bp.s3 = (const float*)s3->dev;
    if (proj) { bp.x0 = x.p; bp.x0_lo = x.lo; } else { bp.x = x.p; bp.x_lo = x.lo; }
    bp.out = out.p; bp.out_lo = out.lo;
    if (t1n) {
      bp.w1p = (const half_t*)w1->dev; bp.w1_lo = (long long)bott * cout; bp.b1 = (const float*)b1->dev; bp.s1 = (const float*)s1->dev;
      bp.t1n = t1n->p; bp.t1n_lo = t1n->lo;
    }
    bp.H = oh; bp.W = ow; bp.Hp = out.Hp(); bp.Wp = out.Wp(); bp.CB = bott / 64;
    Stage& st = add_stage(name, flops, bytes, &bp.sat);
    st.fn = [bp, mpi](int n, hipStream_t s) mutable { bp.M = n * mpi; g_last_conv_variant = 23; return launch_bneck_tail_split(bp, s); };
  }
  return RS_OK;
}

// ---- FPN: laterals + top-down path, output convs, p6
int rs_engine::build_fpn(Graph& g) {
  const int NB = max_batch;
  Act inner[4];
  Act* P = g.P;
  const Act* res_out = g.res_out;
  const bool merge = merge_maps();
  std::vector<DeferredConv> fpn_out(4);
  int rc;
  for (int l = 3; l >= 0; --l) {
    const std::string ln = std::to_string(l + 2);
    if ((rc = new_act(&inner[l], "inner" + ln, NB, res_out[l].H, res_out[l].W, 256, 1))) return rc;
    if ((rc = new_act(&P[l], "p" + ln, NB, res_out[l].H, res_out[l].W, 256, 1))) return rc;
    ConvDesc lat{1, 1, 0, false};
    lat.up = l < 3 ? &inner[l + 1] : nullptr;
    if ((rc = add_conv("fpn_lateral" + ln, "backbone.fpn_lateral" + ln, res_out[l], inner[l], lat))) return rc;
    ConvDesc o{3, 1, 1, false};
    o.defer = merge ? &fpn_out[l] : nullptr;
    if ((rc = add_conv("fpn_output" + ln, "backbone.fpn_output" + ln, inner[l], P[l], o))) return rc;
  }
  // the four output convolutions depend on the laterals only: one launch, largest map first
  if (merge && (rc = add_merged_convs("fpn_output2-5", fpn_out))) return rc;
  const int h6 = (P[3].H - 1) / 2 + 1, w6 = (P[3].W - 1) / 2 + 1;
  if ((rc = new_act(&P[4], "p6", NB, h6, w6, 256, 1))) return rc;
  const Act a = P[3], b = P[4];
  const bool f = f32, sp = split;
  add_stage("fpn.p6", 0, 0).fn = [a, b, f, sp](int n, hipStream_t s) {
    if (sp) return launch_subsample2_split(a.p, a.lo, b.p, b.lo, n, a.H, a.W, b.H, b.W, 256, s);
    return f ? launch_subsample2_f32((const float*)a.p, (float*)b.p, n, a.H, a.W, b.H, b.W, 256, s)
             : launch_subsample2(a.p, b.p, n, a.H, a.W, b.H, b.W, 256, s);
  };
  return RS_OK;
}

// rs_spec.batched_nms = 1: the NMS stage decides torchvision's size rule per image in its own prologue (NmsParams::rule) and leaves the decision
// in two tensors.  Decided on the device: launches, grids and a captured graph are the same for both outcomes and for both modes.
int rs_engine::add_nms_rule(const char* head, NmsParams* np, int group) {
  int rc;
  if ((rc = new_tensor(&np->rule, std::string(head) + "_nms_rule", DT_I32, {max_batch, 2}))) return rc;
  if ((rc = new_tensor(&np->unit, std::string(head) + "_nms_unit", DT_F32, {max_batch}))) return rc;
  np->group = group;
  return RS_OK;
}

// ---- RPN head + proposals
int rs_engine::build_rpn(Graph& g) {
  const rs_spec& S = spec;
  const int NB = max_batch;
  const Act* P = g.P;
  const bool merge = merge_maps();
  const int A = S.num_anchors, L = S.num_levels;
  const int head_cs = (5 * A + 15) / 16 * 16;
  int rc;
  RpnParams rp;
  memset(&rp, 0, sizeof rp);
  std::vector<DeferredConv> rpn_conv(L);
  for (int l = 0; l < L; ++l) {
    if ((rc = new_tensor(&g.rpn_ho[l], "rpn_head" + std::to_string(l + 2), DT_F32, {NB, P[l].H, P[l].W, head_cs}))) return rc;
  }
  // inference engines: the 16-row head runs inside the epilogue of the merged 3x3 launch (conv_deep.hip, ConvParams::head_w), so the
  // 256-channel "rpn_conv" maps are never written
  const BlobEntry* headsp = findw("proposal_generator.rpn_head.headsp");
  const BlobEntry* headsp_si = split ? find("proposal_generator.rpn_head.headsp.wsi") : nullptr;
  const bool fuse_heads = merge && !frozen_fusions_only && rs_debug().fuse_rpn_heads && head_cs == 16 && headsp != nullptr && (!split || headsp_si != nullptr);
  for (int l = 0; l < L; ++l) {
    const std::string ln = std::to_string(l + 2);
    Act& t = g.rpn_t[l];
    if ((rc = new_act(&t, "rpn_conv" + ln, NB, P[l].H, P[l].W, 256, 1))) return rc;   // halo 1: its gradient is the input of a 3x3 (training)
    ConvDesc d{3, 1, 1, true};
    d.defer = merge ? &rpn_conv[l] : nullptr;
    if ((rc = add_conv("rpn.conv" + ln, "proposal_generator.rpn_head.conv", P[l], t, d))) return rc;
    if (merge && fuse_heads) {
      const BlobEntry* hb = find("proposal_generator.rpn_head.heads.b");
      RS_CHECK(hb && wrows(headsp) == 16 && (int)headsp->dims[1] == 256, RS_ERR_BLOB, "rpn head weights (chained order) missing or not 16 x 256");
      rpn_conv[l].p.head_w = (const half_t*)headsp->dev; rpn_conv[l].p.head_b = (const float*)hb->dev; rpn_conv[l].p.head_out = g.rpn_ho[l];
      if (split) { rpn_conv[l].p.head_w_lo = 16 * 256; rpn_conv[l].p.head_scale = (const float*)headsp_si->dev; }
      rpn_conv[l].flops += 2.0 * P[l].H * P[l].W * 256 * 5 * A;
      rpn_conv[l].bytes += (double)P[l].H * P[l].W * (head_cs * 4 - 256 * 2 * planes());       // the heads' output instead of the 256-channel map
    }
    if (merge && l == L - 1 && (rc = add_merged_convs(fuse_heads ? "rpn.conv+heads2-6" : "rpn.conv2-6", rpn_conv))) return rc;
  }
  for (int l = 0; l < L; ++l) {
    const Act t = g.rpn_t[l];
    float* ho = g.rpn_ho[l];
    // 1x1 heads (objectness + deltas fused), fp32 out
    if (!fuse_heads) {
      const BlobEntry* w = findw("proposal_generator.rpn_head.heads");
      const BlobEntry* b = find("proposal_generator.rpn_head.heads.b");
      RS_CHECK(w && b, RS_ERR_BLOB, "rpn head weights missing");
      RS_CHECK(wrows(w) == head_cs, RS_ERR_BLOB, "rpn head rows %d != %d", wrows(w), head_cs);
      ConvParams p;
      memset(&p, 0, sizeof p);
      if ((rc = set_split(&p, "proposal_generator.rpn_head.heads", w, &t, nullptr, nullptr, nullptr, nullptr))) return rc;
      p.in = t.p; p.w = (const half_t*)w->dev; p.bias = (const float*)b->dev; p.out = ho;
      p.Ho = t.H; p.Wo = t.W; p.in_Hp = t.Hp(); p.in_Wp = t.Wp(); p.in_Cs = 256; p.in_off = t.pad; p.stride = 1;
      p.KH = p.KW = 1; p.Cin = 256; p.Kpad = (int)w->dims[1]; p.Cout = head_cs;
      p.out_Hp = t.H; p.out_Wp = t.W; p.out_Cs = head_cs; p.out_pad = 0; p.out_f32 = 1;
      const int mpi = t.H * t.W;
      Stage& st = add_stage("rpn.heads" + std::to_string(l + 2), 2.0 * mpi * 256 * 5 * A, (double)mpi * (256 * 2 + head_cs * 4));
      st.fn = conv_stage_fn(p, mpi, 2, use_glds);
    }
    rp.head[l] = ho;
    rp.H[l] = P[l].H; rp.W[l] = P[l].W; rp.stride[l] = 4 << l;
    uint32_t* keys = nullptr;
    if ((rc = alloc((void**)&keys, (size_t)NB * P[l].H * P[l].W * A * 4 * 2))) return rc;   // keys + candidate list
    rp.keys[l] = keys;
    for (int a = 0; a < A; ++a)
      for (int d = 0; d < 4; ++d) rp.base[l][a][d] = S.cell_anchors[l][a][d];
    RS_CHECK((long long)P[l].H * P[l].W * A < (1 << 24), RS_ERR_UNSUPPORTED, "feature map too large for the RPN index select");
  }
  rp.offset = S.anchor_offset; rp.L = L; rp.A = A; rp.cs = head_cs; rp.topk = S.rpn_pre_nms_topk;
  rp.img_h = (float)net_h; rp.img_w = (float)net_w;
  rp.wx = S.rpn_bbox_reg_weights[0]; rp.wy = S.rpn_bbox_reg_weights[1]; rp.ww = S.rpn_bbox_reg_weights[2]; rp.wh = S.rpn_bbox_reg_weights[3];
  rp.scale_clamp = S.scale_clamp; rp.min_size = S.rpn_min_size;
  uint8_t* cand_keep = nullptr;
  if ((rc = new_tensor(&rp.cand_boxes, "rpn_cand_boxes", DT_F32, {NB, L, 1024, 4}))) return rc;
  if ((rc = new_tensor(&rp.cand_scores, "rpn_cand_scores", DT_F32, {NB, L, 1024}))) return rc;
  if ((rc = new_tensor(&rp.cand_valid, "rpn_cand_valid", DT_U8, {NB, L, 1024}))) return rc;
  if ((rc = new_tensor(&rp.cand_count, "rpn_cand_count", DT_I32, {NB, L}))) return rc;
  if ((rc = new_tensor(&rp.cand_index, "rpn_cand_index", DT_I32, {NB, L, 1024}))) return rc;
  if ((rc = new_tensor(&cand_keep, "rpn_cand_keep", DT_U8, {NB, L, 1024}))) return rc;
  add_stage("rpn.select_decode", 0, 0).fn = [rp](int n, hipStream_t s) mutable { rp.N = n; return launch_rpn_select(rp, s); };
  {
    NmsParams np = {};
    np.boxes = rp.cand_boxes; np.count = rp.cand_count; np.valid = rp.cand_valid; np.keep = cand_keep; np.cap = 1024;
    np.thresh = S.rpn_nms_thresh;
    // suppression masks in global memory for launches of few segments (batch 1-3: launch_nms shares a segment's mask build between workgroups)
    if ((rc = alloc((void**)&np.scratch, (size_t)(NB * L < 32 ? NB * L : 32) * 1024 * 16 * 8))) return rc;
    if (S.batched_nms) { if ((rc = add_nms_rule("rpn", &np, L))) return rc; }
    add_stage("rpn.nms", 0, 0).fn = [np, L](int n, hipStream_t s) { return launch_nms(np, n * L, s); };
  }
  const int PC = 1024;   // proposal slots per image
  float* prop_scores;
  if ((rc = new_tensor(&g.prop_boxes, "proposal_boxes", DT_F32, {NB, PC, 4}))) return rc;
  if ((rc = new_tensor(&prop_scores, "proposal_logits", DT_F32, {NB, PC}))) return rc;
  if ((rc = new_tensor(&g.prop_level, "proposal_level", DT_I32, {NB, PC}))) return rc;
  if ((rc = new_tensor(&g.prop_count, "proposal_count", DT_I32, {NB}))) return rc;
  // visiting order of box.roi_align (RpnMergeParams::prop_order): inference engines on the windowed fp16 kernel only -- a training
  // engine overwrites the proposal buffer with its sampled RoIs after this stage
  const bool roi_order = !f32 && !(split && rs_debug().roi_window != 1) && !frozen_fusions_only && rs_debug().roi_order != 0;
  if (roi_order) {
    if ((rc = new_tensor(&g.prop_order, "proposal_order", DT_I32, {NB, PC}))) return rc;
  }
  RpnMergeParams mp = {};
  mp.cand_boxes = rp.cand_boxes; mp.cand_scores = rp.cand_scores; mp.keep = cand_keep; mp.cand_count = rp.cand_count;
  mp.L = L; mp.post_topk = S.rpn_post_nms_topk; mp.cap = PC;
  mp.prop_boxes = g.prop_boxes; mp.prop_scores = prop_scores; mp.prop_level = g.prop_level; mp.prop_count = g.prop_count;
  mp.prop_order = g.prop_order;
  add_stage("rpn.merge", 0, 0).fn = [mp](int n, hipStream_t s) { return launch_rpn_merge(mp, n, s); };
  return RS_OK;
}

// the pyramid levels both RoIAligns read
RoiAlignParams rs_engine::roi_align_levels(const Graph& g) const {
  RoiAlignParams ra;
  memset(&ra, 0, sizeof ra);
  for (int l = 0; l < 4; ++l) { ra.feat[l] = g.P[l].p; ra.H[l] = g.P[l].H; ra.W[l] = g.P[l].W; ra.scale[l] = 1.0f / (float)(4 << l); }
  ra.nlevels = 4; ra.C = 256; ra.f32 = prec_code();
  for (int l = 0; l < 4; ++l) ra.feat_lo[l] = g.P[l].lo;
  return ra;
}

// ---- box head + detections
int rs_engine::build_box_head(Graph& g) {
  const rs_spec& S = spec;
  const int NB = max_batch, PC = 1024;
  const int PR = S.box_pooler_resolution;
  int rc;
  Act boxfeat;   // [NB*PC] "images" of PR x PR x 256
  if ((rc = new_act(&boxfeat, "box_pooled", NB * PC, PR, PR, 256, 0))) return rc;
  int* box_level = nullptr;
  if ((rc = new_tensor(&box_level, "box_roi_level", DT_I32, {NB, PC}))) return rc;
  {
    RoiAlignParams q = roi_align_levels(g);
    q.rois = g.prop_boxes; q.per_image_count = g.prop_count; q.slots_per_image = PC; q.out = boxfeat.p; q.out_lo = boxfeat.lo; q.P = PR; q.out_pad = 0;
    q.out_level = box_level;
    q.order = g.prop_order;
    add_stage("box.roi_align", 0, (double)PC * PR * PR * 256 * 2 * 2 * planes()).fn =
        [q](int n, hipStream_t s) mutable { q.S = n * PC; return launch_roi_align(q, s); };
  }
  // FC layers as 1x1 "convs" over a (M x 1) image
  const int FC = S.box_fc_dim;
  Act fin, f1, f2;
  fin.p = boxfeat.p; fin.lo = boxfeat.lo; fin.N = 1; fin.H = NB * PC; fin.W = 1; fin.C = PR * PR * 256; fin.pad = 0;
  if ((rc = new_act(&f1, "box_fc1", 1, NB * PC, 1, FC, 0))) return rc;
  if ((rc = new_act(&f2, "box_fc2", 1, NB * PC, 1, FC, 0))) return rc;
  auto add_fc = [&](const std::string& name, const std::string& wn, const Act& in, const Act& out, bool relu, float* out32, int rows32) -> int {
    const BlobEntry* w = findw(wn);
    const BlobEntry* b = find(wn + ".b");
    RS_CHECK(w && b, RS_ERR_BLOB, "weights for %s missing", wn.c_str());
    ConvParams p;
    memset(&p, 0, sizeof p);
    { int rc2 = set_split(&p, wn, w, &in, out32 ? nullptr : &out, nullptr, nullptr, nullptr); if (rc2) return rc2; }
    p.in = in.p; p.w = (const half_t*)w->dev; p.bias = (const float*)b->dev;
    p.Ho = NB * PC; p.Wo = 1; p.in_Hp = NB * PC; p.in_Wp = 1; p.in_Cs = in.C; p.stride = 1; p.KH = p.KW = 1; p.Cin = in.C;
    p.Kpad = (int)w->dims[1];
    p.out_Hp = NB * PC; p.out_Wp = 1; p.relu = relu;
    if (out32) { p.out = out32; p.Cout = rows32; p.out_Cs = rows32; p.out_f32 = 1; }
    else { p.out = out.p; p.Cout = out.C; p.out_Cs = out.C; }
    RS_CHECK(wrows(w) >= p.Cout && p.Kpad >= in.C, RS_ERR_BLOB, "%s: weight shape", wn.c_str());
    const int variant = out32 ? 2 : -1;
    Stage& st = add_stage(name, 2.0 * PC * (double)in.C * p.Cout, (double)PC * (in.C * 2 * planes() + p.Cout * (out32 ? 4 : 2 * planes())),
                          out32 ? nullptr : &p.sat);
    st.fn = conv_stage_fn(p, PC, variant, use_glds);
    return RS_OK;
  };
  if ((rc = add_fc("box.fc1", "roi_heads.box_head.fc1", fin, f1, true, nullptr, 0))) return rc;
  if ((rc = add_fc("box.fc2", "roi_heads.box_head.fc2", f1, f2, true, nullptr, 0))) return rc;
  const int K = S.num_classes;
  const int pred_cs = (5 * K + 1 + 15) / 16 * 16;
  if ((rc = new_tensor(&g.pred, "box_pred", DT_F32, {NB, PC, pred_cs}))) return rc;
  if ((rc = add_fc("box.predictor", "roi_heads.box_predictor", f2, f2, false, g.pred, pred_cs))) return rc;

  D = S.detections_per_image;
  BoxCandParams bc;
  memset(&bc, 0, sizeof bc);
  bc.pred = g.pred; bc.prop_boxes = g.prop_boxes; bc.prop_count = g.prop_count; bc.K = K; bc.cap = PC; bc.cs = pred_cs;
  bc.wx = S.box_reg_weights[0]; bc.wy = S.box_reg_weights[1]; bc.ww = S.box_reg_weights[2]; bc.wh = S.box_reg_weights[3];
  bc.scale_clamp = S.scale_clamp; bc.img_h = (float)net_h; bc.img_w = (float)net_w; bc.score_thresh = S.score_thresh_test;
  uint8_t* seg_keep = nullptr;
  if (K > RS_DET_GROUP) {   // many classes: softmax statistics per RoI, computed once (launch_box_candidates)
    if ((rc = new_tensor(&bc.roi_stat, "box_roi_stat", DT_F32, {NB, PC, 2}))) return rc;
  }
  if ((rc = new_tensor(&bc.dec_boxes, "box_dec_boxes", DT_F32, {NB, PC, K, 4}))) return rc;
  if ((rc = new_tensor(&bc.dec_scores, "box_dec_scores", DT_F32, {NB, PC, K}))) return rc;
  if ((rc = new_tensor(&bc.seg_boxes, "box_seg_boxes", DT_F32, {NB, K, 1024, 4}))) return rc;
  if ((rc = new_tensor(&bc.seg_roi, "box_seg_roi", DT_I32, {NB, K, 1024}))) return rc;
  if ((rc = new_tensor(&bc.seg_count, "box_seg_count", DT_I32, {NB, K}))) return rc;
  if ((rc = new_tensor(&seg_keep, "box_seg_keep", DT_U8, {NB, K, 1024}))) return rc;
  add_stage("box.candidates", 0, 0).fn = [bc](int n, hipStream_t s) { return launch_box_candidates(bc, n, s); };
  {
    NmsParams np = {};
    np.boxes = bc.seg_boxes; np.count = bc.seg_count; np.valid = nullptr; np.keep = seg_keep; np.cap = 1024; np.thresh = S.nms_thresh_test;
    if ((rc = alloc((void**)&np.scratch, (size_t)(NB * K < 32 ? NB * K : 32) * 1024 * 16 * 8))) return rc;
    if (S.batched_nms) { if ((rc = add_nms_rule("box", &np, K))) return rc; }
    add_stage("box.nms", 0, 0).fn = [np, K](int n, hipStream_t s) { return launch_nms(np, n * K, s); };
  }
  int* det_roi = nullptr;
  if ((rc = new_tensor(&det_boxes_net, "det_boxes_net", DT_F32, {NB, D, 4}))) return rc;
  if ((rc = new_tensor(&det_boxes, "det_boxes", DT_F32, {NB, D, 4}))) return rc;
  if ((rc = new_tensor(&det_scores, "det_scores", DT_F32, {NB, D}))) return rc;
  if ((rc = new_tensor(&det_classes, "det_classes", DT_I32, {NB, D}))) return rc;
  if ((rc = new_tensor(&det_roi, "det_roi", DT_I32, {NB, D}))) return rc;
  if ((rc = new_tensor(&det_count, "det_count", DT_I32, {NB}))) return rc;
  DetMergeParams dm;
  memset(&dm, 0, sizeof dm);
  dm.dec_boxes = bc.dec_boxes; dm.dec_scores = bc.dec_scores; dm.seg_roi = bc.seg_roi; dm.seg_count = bc.seg_count; dm.keep = seg_keep;
  dm.K = K; dm.cap = PC; dm.dets_per_image = D;
  dm.scale_x = (float)((double)tile_w / (double)net_w);
  dm.scale_y = (float)((double)tile_h / (double)net_h);
  dm.out_w = (float)tile_w; dm.out_h = (float)tile_h;
  dm.det_boxes_net = det_boxes_net; dm.det_boxes = det_boxes; dm.det_scores = det_scores; dm.det_classes = det_classes;
  dm.det_roi = det_roi; dm.det_count = det_count;
  if (K > RS_DET_GROUP) {   // many classes: the groups' partial winners between the merge's two launches (launch_det_merge)
    const int G = det_merge_groups(K);
    if ((rc = alloc((void**)&dm.part_keys, (size_t)NB * G * D * 8))) return rc;
    if ((rc = alloc((void**)&dm.part_count, (size_t)NB * G * 4))) return rc;
  }
  add_stage("box.merge_postprocess", 0, 0).fn = [dm](int n, hipStream_t s) { return launch_det_merge(dm, n, s); };
  return RS_OK;
}

// ---- mask head: RoIAlign of the detections, 4 x conv 3x3, deconv 2x2 s2 + predictor + sigmoid, paste into the tile
int rs_engine::build_mask_head(Graph& g) {
  const rs_spec& S = spec;
  const int NB = max_batch, Dc = D;
  const int MR = S.mask_pooler_resolution, R = NB * D;
  int rc;
  if ((rc = new_tensor(&g.slot_list, "det_slot_list", DT_I32, {R}))) return rc;
  if ((rc = new_tensor(&g.det_total, "det_total", DT_I32, {1}))) return rc;
  int *slot_list = g.slot_list, *det_total = g.det_total;
  {
    int* dc = det_count;
    add_stage("mask.compact", 0, 0).fn = [dc, Dc, slot_list, det_total](int n, hipStream_t s) { return launch_det_compact(dc, n, Dc, slot_list, det_total, s); };
  }
  Act mx;
  if ((rc = new_act(&mx, "mask_pooled", R, MR, MR, 256, 1))) return rc;
  {
    RoiAlignParams q = roi_align_levels(g);
    q.rois = det_boxes_net; q.slot_list = slot_list; q.n_entries = det_total; q.slots_per_image = D;
    q.out = mx.p; q.out_lo = mx.lo; q.P = MR; q.out_pad = 1;
    add_stage("mask.roi_align", 0, (double)D * MR * MR * 256 * 2 * 2 * planes()).fn =
        [q, Dc](int n, hipStream_t s) mutable { q.S = n * Dc; return launch_roi_align(q, s); };
  }
  Act curm = mx;
  for (int i = 0; i < S.mask_num_conv; ++i) {
    Act o;
    const std::string nm = "mask_fcn" + std::to_string(i + 1);
    if ((rc = new_act(&o, nm, R, MR, MR, 256, 1))) return rc;
    ConvDesc d{3, 1, 1, true};
    d.units_per_tile = D; d.m_count = det_total;
    if ((rc = add_conv("mask.fcn" + std::to_string(i + 1), "roi_heads.mask_head." + nm, curm, o, d))) return rc;
    curm = o;
  }
  if ((rc = new_tensor(&mask_probs, "mask_probs", DT_F32, {NB, D, RS_MASK_SIDE, RS_MASK_SIDE}))) return rc;
  const BlobEntry* dw = findw("roi_heads.mask_head.deconv");
  const BlobEntry* db = find("roi_heads.mask_head.deconv.b");
  const BlobEntry* pw = find("roi_heads.mask_head.predictor.w");
  const BlobEntry* pb = find("roi_heads.mask_head.predictor.b");
  RS_CHECK(dw && db && wrows(dw) == 1024, RS_ERR_BLOB, "deconv weights missing / wrong rows");
  RS_CHECK(pw && pb && pw->dtype == DT_F32, RS_ERR_BLOB, "mask predictor weights missing");
  const bool fuse = f32 ? false : rs_debug().fuse_mask_predictor != 0;
  ConvParams dp;
  memset(&dp, 0, sizeof dp);
  if ((rc = set_split(&dp, "roi_heads.mask_head.deconv", dw, &curm, nullptr, nullptr, nullptr, nullptr))) return rc;
  dp.in = curm.p; dp.w = (const half_t*)dw->dev; dp.bias = (const float*)db->dev;
  dp.Ho = MR; dp.Wo = MR; dp.in_Hp = curm.Hp(); dp.in_Wp = curm.Wp(); dp.in_Cs = 256; dp.in_off = 1; dp.stride = 1; dp.KH = dp.KW = 1;
  dp.Cin = 256; dp.Kpad = (int)dw->dims[1]; dp.Cout = 256; dp.out_Hp = 2 * MR; dp.out_Wp = 2 * MR; dp.out_Cs = 256; dp.out_pad = 0; dp.relu = 1;
  dp.m_count = det_total; dp.m_mul = MR * MR;
  const int per_roi = MR * MR;
  const int glds = use_glds;
  MaskPredictParams mp = {};
  mp.b = (const float*)pb->dev; mp.slot_list = slot_list; mp.det_classes = det_classes;
  mp.n_entries = det_total; mp.out = mask_probs; mp.S = RS_MASK_SIDE;
  if (fuse) {
    // deconv 2x2 s2 + ReLU + predictor 1x1 (predicted class only) in one launch: the 28x28x256 map (40 MB per
    // tile) is never written; a small kernel then adds the class bias and applies the sigmoid in place.
    dp.mode = 2; dp.out = nullptr;
    dp.dot_w = (const float*)pw->dev; dp.dot_cls = det_classes; dp.dot_slot = slot_list; dp.dot_out = mask_probs;
    dp.dot_k = (int)pw->dims[0];
    const bool sp = split;
    float* probs = mask_probs;
    const size_t zero_per_tile = (size_t)D * RS_MASK_SIDE * RS_MASK_SIDE * 4;
    add_stage("mask.deconv_predict", 2.0 * D * per_roi * 256 * 1024 + 2.0 * D * RS_MASK_SIDE * RS_MASK_SIDE * 256,
              (double)D * per_roi * 256 * 2 * planes() + (double)D * RS_MASK_SIDE * RS_MASK_SIDE * 4).fn =
        [dp, per_roi, Dc, glds, probs, zero_per_tile, sp](int n, hipStream_t s) mutable {
      dp.M = n * Dc * per_roi;
      // conv_wreg.hip (22: persistent, a (dy, dx) group's weights in registers) or conv_igemm's tile where one workgroup holds all 256
      // channels of a group (14 / 10); the two give the same bits.  Split mode: conv_wide1x1_split.hip (28) from the rule's pixel count on, which
      // STORES every logit that mask.bias_sigmoid and mask.paste read (the entries below the device-side count) -- no zeroing, no atomics; same bits again
      const int dv = rs_debug().deconv_variant;
      int force = (dv == 22 && (sp || !(rs_debug().conv_wreg && glds > 0))) ? 14 : dv;
      if (dv == 22 && sp) {      // the rule's answer for the split mode: 28 or 14 (conv_choose_variant)
        ConvParams probe = dp;
        force = conv_choose_variant(probe, -1, glds);
      }
      if (!(force >= 28 && force <= 31)) RS_HIP(hipMemsetAsync(probs, 0, zero_per_tile * n, s));
      return launch_conv(dp, s, force, glds);
    };
    mp.f32 = 0;
    mp.in = nullptr; mp.w = nullptr;
    add_stage("mask.bias_sigmoid", 0, 0).fn = [mp, Dc](int n, hipStream_t s) { return launch_mask_sigmoid(mp, n * Dc, s); };
  } else {
    Act dec;
    if ((rc = new_act(&dec, "mask_deconv", R, 2 * MR, 2 * MR, 256, 0))) return rc;
    dp.mode = 1; dp.out = dec.p; dp.out_lo = dec.lo;
    Stage& st = add_stage("mask.deconv", 2.0 * D * per_roi * 256 * 1024, (double)D * per_roi * 256 * 2 * 5, &dp.sat);
    st.fn = [dp, per_roi, Dc, glds](int n, hipStream_t s) mutable { dp.M = n * Dc * per_roi; return launch_conv(dp, s, -1, glds); };
    mp.in = dec.p; mp.w = (const float*)pw->dev; mp.f32 = prec_code(); mp.in_lo = dec.lo;
    add_stage("mask.predict_sigmoid", 0, (double)D * RS_MASK_SIDE * RS_MASK_SIDE * (256 * 2 + 4)).fn =
        [mp, Dc](int n, hipStream_t s) { return launch_mask_predict(mp, n * Dc, s); };
  }
  const int Wb = (tile_w + 7) / 8;
  if ((rc = new_tensor(&masks, "masks", DT_U8, {NB, D, tile_h, Wb}))) return rc;
  if ((rc = alloc((void**)&crop_data, (size_t)R * tile_h * Wb))) return rc;
  if ((rc = alloc((void**)&crop_rects, (size_t)R * 16))) return rc;
  if ((rc = alloc((void**)&crop_offsets, (size_t)R * 4))) return rc;
  if ((rc = alloc((void**)&crop_total, 16))) return rc;
  PasteParams pm;
  pm.probs = mask_probs; pm.det_boxes = det_boxes; pm.slot_list = slot_list; pm.n_entries = det_total; pm.out = masks;
  pm.S = RS_MASK_SIDE; pm.out_h = tile_h; pm.out_w = tile_w; pm.threshold = S.mask_threshold;
  add_stage("mask.paste", 0, (double)D * tile_h * Wb).fn = [pm, Dc](int n, hipStream_t s) { return launch_paste_masks(pm, n * Dc, s); };
  return RS_OK;
}

// Phase and stream of every stage.  With RS_SIDE_STREAM=1 (default) the detection glue runs on a side stream:
// alone it changes nothing (the hand-off events keep the order), but two engines that share the wide stream can
// then hide one batch's glue behind the other batch's convolutions (rs_engine_infer_phase).
int rs_engine::assign_phases() {
  const bool side = rs_debug().side_stream != 0 && !use_graph;
  static const char* kNarrow[] = {"rpn.select_decode", "rpn.nms", "rpn.merge", "box.candidates", "box.nms",
                                  "box.merge_postprocess", "mask.compact"};
  int phase = 0;
  const bool roi_narrow = rs_debug().narrow_roialign != 0;
  for (Stage& st : stages) {
    if (st.name.rfind("box.", 0) == 0 && phase < 1) phase = 1;
    if (st.name.rfind("mask.", 0) == 0 && st.name != "mask.compact" && phase < 2) phase = 2;
    st.phase = phase;
    for (const char* nm : kNarrow) if (side && st.name == nm) st.narrow = true;
    // RoIAlign is gather-bound (L1/L2 request rate), not MFMA-bound: with RS_NARROW_ROIALIGN=1 it runs on the side stream and
    // shares the chip with the other lane's convolutions (+1 % tiles/s measured).  Off by default: the convolutions it
    // overlaps run ~12 % longer each, which blurs the per-kernel roofline measurement for a 1 % gain.
    if (side && roi_narrow && (st.name == "box.roi_align" || st.name == "mask.roi_align")) st.narrow = true;
    // (measured and left on the wide stream: mask.paste, preprocess, box.predictor, mask.bias_sigmoid -- 0 to -1 %)
  }
  if (!side) return RS_OK;
  RS_HIP(hipStreamCreateWithFlags(&narrow, hipStreamNonBlocking));
  RS_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
  bool prev = false;
  for (Stage& st : stages) {
    if (st.narrow != prev) RS_HIP(hipEventCreateWithFlags(&st.handoff, hipEventDisableTiming));
    prev = st.narrow;
  }
  return RS_OK;
}

int rs_engine::run_stages(int n, bool record, int phase, bool all_wide) {
  if (sat_dev && phase <= 0) RS_HIP(hipMemsetAsync(sat_dev, 0, stages.size() * 8, stream));   // a forward starts: its counters from zero
  for (size_t si = 0; si < stages.size(); ++si) {
    Stage& st = stages[si];
    if (phase >= 0 && st.phase != phase) continue;
    if (all_wide) {                     // one-tile graph capture: every stage on the wide stream, in list order (the side stream hides nothing at one tile)
      g_last_conv_variant = -2;
      int rc = st.fn(n, stream);
      if (rc) return rc;
      st.variant = g_last_conv_variant;
      continue;
    }
    if (st.narrow != on_narrow) {       // hand the dependency chain over to the other stream
      hipStream_t from = on_narrow ? narrow : stream, to = st.narrow ? narrow : stream;
      RS_HIP(hipEventRecord(st.handoff, from));
      RS_HIP(hipStreamWaitEvent(to, st.handoff, 0));
      on_narrow = st.narrow;
    }
    hipStream_t ss = st.narrow ? narrow : stream;
    const bool pooled = record && profiling >= 2 && ev_used < ev_pool.size();
    if (record && profiling == 1) RS_HIP(hipEventRecord(ev0, ss));
    if (pooled) RS_HIP(hipEventRecord(ev_pool[ev_used].first, ss));
    g_last_conv_variant = -2;
    int rc = st.fn(n, ss);
    if (rc) return rc;
    st.variant = g_last_conv_variant;
    if (pooled) {
      RS_HIP(hipEventRecord(ev_pool[ev_used].second, ss));
      ev_stage[ev_used] = (int)si;
      ev_batch[ev_used] = n;
      ++ev_used;
    }
    if (record && profiling == 1) {
      RS_HIP(hipEventRecord(ev1, ss));
      RS_HIP(hipEventSynchronize(ev1));
      float ms = 0.f;
      RS_HIP(hipEventElapsedTime(&ms, ev0, ev1));
      st.ms_total += ms;
      st.calls += 1;
      st.last_flops = st.flops_per_image * n;
      st.last_bytes = st.bytes_per_image * n;
    }
  }
  if ((phase < 0 || phase == RS_NUM_PHASES - 1) && on_narrow) {   // the forward ended on the side stream: join
    RS_HIP(hipEventRecord(ev_join, narrow));
    RS_HIP(hipStreamWaitEvent(stream, ev_join, 0));
    on_narrow = false;
  }
  if (sat_dev && (phase < 0 || phase == RS_NUM_PHASES - 1))      // the forward is complete: what the fetches copy
    RS_HIP(hipMemcpyAsync(sat_snap, sat_dev, stages.size() * 8, hipMemcpyDeviceToDevice, stream));
  return RS_OK;
}

// One forward.  The ~110 launches of a forward are replayed from a hipGraph (captured per batch size
// after one eager warm-up run, which also performs the one-time hipFuncSetAttribute calls); forwards
// that are being event-profiled run eagerly so every launch can be bracketed.
int rs_engine::run(const uint8_t* tiles, int n, int phase) {
  RS_CHECK(n >= 1 && n <= max_batch, RS_ERR_ARG, "batch %d outside [1, %d]", n, max_batch);
  RS_CHECK(phase >= -1 && phase < RS_NUM_PHASES, RS_ERR_ARG, "phase %d outside [-1, %d)", phase, RS_NUM_PHASES);
  if (phase <= 0) {
    if (tiles != tiles_dev) {
      // tiles already resident elsewhere on the device: stage them into the engine's input buffer
      { int rc = wait_band_tiles(); if (rc) return rc; }
      RS_HIP(hipMemcpyAsync(tiles_dev, tiles, (size_t)n * tile_h * tile_w * tile_c, hipMemcpyDeviceToDevice, stream));
    }
    const long long idx = forward_index++;
    cur_record = profiling == 1 || profiling == 2 || (profiling == 3 && (idx & 3) == 0);
  }
  if (copy_pending && (phase < 0 || phase == 1)) {
    // the box head rewrites the result buffers: let an outstanding rs_engine_fetch_async of the previous forward finish first
    RS_HIP(hipStreamWaitEvent(stream, ev_copied, 0));
    copy_pending = false;
  }
  const bool record = cur_record;
  // One tile per call (what the reference's predictor(im) loop submits): the ~110 launches replay from a hipGraph captured with every stage on the wide
  // stream -- same kernels, same order, same bits; 2.25 -> 2.13 ms fp16, 3.76 -> 3.67 ms split (tools/ubench/single_tile_latency.py).  Larger batches stay eager.
  // (inference engines on the one network geometry only: a trainer's forward engine re-reads host state per step -- per-image sizes, their resize tables)
  const bool small = n == 1 && rs_debug().graph_small != 0 && !on_narrow && img_new_h.empty() && !frozen_fusions_only;
  if (phase >= 0 || record || !(use_graph || small) || !warmed.count(n)) {
    int rc = run_stages(n, record, phase);
    if (rc) return rc;
    if (phase < 0) warmed.insert(n);
    return RS_OK;
  }
  auto it = graphs.find(n);
  if (it == graphs.end()) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    RS_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    int rc = run_stages(n, false, -1, !use_graph);
    hipError_t he = hipStreamEndCapture(stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    RS_HIP(he);
    RS_HIP(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    it = graphs.emplace(n, ge).first;
  }
  RS_HIP(hipGraphLaunch(it->second, stream));
  return RS_OK;
}

int rs_engine::resolve_profile() {
  if (ev_used == 0) return RS_OK;
  RS_HIP(hipStreamSynchronize(stream));
  if (narrow) RS_HIP(hipStreamSynchronize(narrow));
  for (size_t i = 0; i < ev_used; ++i) {
    float ms = 0.f;
    RS_HIP(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
    Stage& st = stages[ev_stage[i]];
    st.ms_total += ms;
    st.calls += 1;
    st.last_flops = st.flops_per_image * ev_batch[i];
    st.last_bytes = st.bytes_per_image * ev_batch[i];
  }
  ev_used = 0;
  return RS_OK;
}

// ---- the steps of a result fetch (rs_engine_fetch and the rs_engine_fetch_*_async / _wait entries)
int rs_engine::ensure_crop_header() {
  if (ev_crop_hdr) return RS_OK;
  RS_HIP(hipEventCreateWithFlags(&ev_crop_hdr, hipEventDisableTiming));
  RS_HIP(hipHostMalloc((void**)&h_crop_total, 16, hipHostMallocDefault));
  return RS_OK;
}

int rs_engine::ensure_polygon_buffers() {
  if (poly_ready) return RS_OK;
  const int inst = max_batch * D;
  size_t b_hdr, b_prc, b_rlen, b_xy;
  polygonize_scratch_bytes(inst, &b_hdr, &b_prc, &b_rlen, &b_xy);
  PolyParams& q = poly;
  memset(&q, 0, sizeof q);
  int rc;
  if ((rc = alloc((void**)&q.s_hdr, b_hdr))) return rc;
  if ((rc = alloc((void**)&q.s_prc, b_prc))) return rc;
  if ((rc = alloc((void**)&q.s_rlen, b_rlen))) return rc;
  if ((rc = alloc((void**)&q.s_xy, b_xy))) return rc;
  if ((rc = alloc((void**)&q.header, (size_t)inst * PG_HDR * 4))) return rc;
  if ((rc = alloc((void**)&q.poly_ring_count, (size_t)inst * PG_RING_CAP * 4))) return rc;
  if ((rc = alloc((void**)&q.ring_len, (size_t)inst * PG_RING_CAP * 4))) return rc;
  if ((rc = alloc((void**)&q.xy, (size_t)inst * PG_VERTEX_CAP * 4))) return rc;
  if ((rc = alloc((void**)&q.totals, 16))) return rc;
  RS_HIP(hipEventCreateWithFlags(&ev_poly_hdr, hipEventDisableTiming));
  RS_HIP(hipHostMalloc((void**)&h_poly_totals, 16, hipHostMallocDefault));
  poly_ready = true;
  return RS_OK;
}

int rs_engine::ensure_eval_buffers() {
  if (eval_pool) return RS_OK;
  MtLayout L;
  mt_layout(max_batch, max_batch * RS_EVAL_GT_CAP, max_batch * 512, (size_t)max_batch * 65536, &L);
  const size_t mask_bytes = (size_t)tile_h * ((tile_w + 7) / 8);
  int rc;
  if ((rc = alloc((void**)&eval_gt_masks, (size_t)max_batch * RS_EVAL_GT_CAP * mask_bytes))) return rc;
  if ((rc = alloc((void**)&eval_inter, (size_t)max_batch * D * RS_EVAL_GT_CAP * 4))) return rc;
  if ((rc = alloc((void**)&eval_det_area, (size_t)max_batch * D * 4))) return rc;
  if ((rc = alloc((void**)&eval_gt_area, (size_t)max_batch * RS_EVAL_GT_CAP * 4))) return rc;
  RS_HIP(hipEventCreateWithFlags(&ev_eval_upload, hipEventDisableTiming));
  RS_HIP(hipHostMalloc((void**)&eval_pinned, L.bytes, hipHostMallocDefault));
  eval_pool_bytes = L.bytes;
  return alloc((void**)&eval_pool, L.bytes);      // last: its presence says that all of the above exists
}

int rs_engine::ensure_match_buffers() {
  if (match_order) return RS_OK;
  const size_t cap = (size_t)max_batch * RS_EVAL_GT_CAP, K = (size_t)spec.num_classes, W = ((size_t)D + 31) / 32;
  const size_t rows = (size_t)max_batch * CM_KINDS * CM_RANGES;
  int rc;
  if ((rc = alloc((void**)&match_gt_boxes, cap * 36))) return rc;    // [cap][4] doubles, then [cap] classes
  if ((rc = alloc((void**)&match_class_first, (size_t)max_batch * (K + 1) * 4))) return rc;
  if ((rc = alloc((void**)&match_gt_per_class, (size_t)max_batch * K * 4))) return rc;
  if ((rc = alloc((void**)&match_matched, rows * CM_THRS * W * 4))) return rc;
  if ((rc = alloc((void**)&match_ignored, rows * CM_THRS * W * 4))) return rc;
  if ((rc = alloc((void**)&match_npig, rows * K * 4))) return rc;
  RS_HIP(hipHostMalloc((void**)&match_pinned, cap * 36, hipHostMallocDefault));
  return alloc((void**)&match_order, (size_t)max_batch * D * 4);     // last: its presence says that all of the above exists
}

int rs_engine::ensure_vote_buffers() {
  if (vote_pairs) return RS_OK;
  vote_cells = (size_t)max_batch * RS_EVAL_GT_CAP * (size_t)spec.num_classes;
  int rc;
  if ((rc = alloc((void**)&vote_wscore, vote_cells * 16))) return rc;        // wscore, then wfrac
  return alloc((void**)&vote_pairs, vote_cells * 4);   // last: its presence says that all of the above exists
}

int rs_engine::ensure_vote_sweep_buffers() {
  if (sweep_pairs) return RS_OK;
  sweep_cells = (size_t)max_batch * RS_VOTE_SWEEP_MAX * RS_EVAL_GT_CAP * (size_t)spec.num_classes;
  int rc;
  if ((rc = alloc((void**)&sweep_wscore, sweep_cells * 16))) return rc;      // wscore, then wfrac
  return alloc((void**)&sweep_pairs, sweep_cells * 4); // last: its presence says that all of the above exists
}

int rs_engine::ensure_poly_vote_buffers() {
  if (pvote_flagged) return RS_OK;
  int rc;
  if ((rc = alloc((void**)&pvote_frac, (size_t)max_batch * D * RS_EVAL_GT_CAP * 8))) return rc;
  if ((rc = alloc((void**)&pvote_area, (size_t)max_batch * RS_EVAL_GT_CAP * 8))) return rc;
  return alloc((void**)&pvote_flagged, (size_t)max_batch * 4);   // last: its presence says that all of the above exists
}

int rs_engine::ensure_band_buffers() {
  if (band_hist_dev) return RS_OK;
  RS_HIP(hipEventCreateWithFlags(&ev_band_tiles, hipEventDisableTiming));
  return alloc((void**)&band_hist_dev, (size_t)max_batch * RS_EVAL_GT_CAP * tile_c * BH_BINS * 4);   // last: its presence says that all of the above exists
}

// The histogram kernel reads tiles_dev on the copy stream; everything that writes tiles_dev does so on `stream` and calls this first.
int rs_engine::wait_band_tiles() {
  if (!band_tiles_pending) return RS_OK;
  RS_HIP(hipStreamWaitEvent(stream, ev_band_tiles, 0));
  band_tiles_pending = false;
  return RS_OK;
}

// upload of the packed pool and the rasteriser: on the copy stream, behind the forward and in front of whatever reads the canvases
int rs_engine::launch_eval_labels(const void* layout, hipStream_t s) {
  const MtLayout& L = *(const MtLayout*)layout;
  RS_HIP(hipMemcpyAsync(eval_pool, eval_pinned, L.bytes, hipMemcpyHostToDevice, s));
  RS_HIP(hipEventRecord(ev_eval_upload, s));
  eval_upload_pending = true;
  CanvasRasterParams q;
  memset(&q, 0, sizeof q);
  q.inst_first = (const int*)(eval_pool + L.o_inst); q.poly_off = (const int*)(eval_pool + L.o_off); q.poly_len = (const int*)(eval_pool + L.o_len);
  q.polys = (const double*)(eval_pool + L.o_xy); q.out = eval_gt_masks; q.n_inst = L.n_inst; q.side = tile_h;
  return launch_canvas_raster(q, s);
}

// the pair counts of the forward's masks against those canvases, in front of the result copies
int rs_engine::launch_eval_pairs(int n, hipStream_t s) {
  PairCountParams c;
  memset(&c, 0, sizeof c);
  c.det_masks = masks; c.det_count = det_count; c.gt_masks = eval_gt_masks; c.tile_first = (const int*)eval_pool;
  c.inter = eval_inter; c.det_area = eval_det_area; c.gt_area = eval_gt_area; c.n = n; c.D = D; c.g_cap = RS_EVAL_GT_CAP;
  c.bytes = (long long)tile_h * ((tile_w + 7) / 8);
  return launch_mask_pair_counts(c, s);
}

int rs_engine::launch_eval_counts(int n, const void* layout, hipStream_t s) {
  { int rc = launch_eval_labels(layout, s); if (rc) return rc; }
  return launch_eval_pairs(n, s);
}

int rs_engine::begin_fetch(hipStream_t* s) {
  if (!copy_stream) {
    RS_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    RS_HIP(hipEventCreateWithFlags(&ev_results, hipEventDisableTiming));
    RS_HIP(hipEventCreateWithFlags(&ev_copied, hipEventDisableTiming));
  }
  RS_HIP(hipEventRecord(ev_results, stream));          // everything enqueued so far for this engine (its last phase included)
  RS_HIP(hipStreamWaitEvent(copy_stream, ev_results, 0));
  *s = copy_stream;
  return RS_OK;
}

int rs_engine::end_fetch(hipStream_t s, hipEvent_t header) {
  { int rc = sat_copy(s); if (rc) return rc; }
  RS_HIP(hipEventRecord(ev_copied, s));
  if (header) RS_HIP(hipEventRecord(header, s));
  copy_pending = true;
  return RS_OK;
}

int rs_engine::enqueue_dets(const rs_dets* o, int n, hipStream_t s, bool want_masks) {
  RS_HIP(hipMemcpyAsync(o->count, det_count, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  if (o->boxes) RS_HIP(hipMemcpyAsync(o->boxes, det_boxes, (size_t)n * D * 16, hipMemcpyDeviceToHost, s));
  if (o->scores) RS_HIP(hipMemcpyAsync(o->scores, det_scores, (size_t)n * D * 4, hipMemcpyDeviceToHost, s));
  if (o->classes) RS_HIP(hipMemcpyAsync(o->classes, det_classes, (size_t)n * D * 4, hipMemcpyDeviceToHost, s));
  if (want_masks && o->masks && masks) RS_HIP(hipMemcpyAsync(o->masks, masks, (size_t)n * D * tile_h * ((tile_w + 7) / 8), hipMemcpyDeviceToHost, s));
  return RS_OK;
}

int rs_engine::launch_crops(int n, hipStream_t s) {
  CropParams cp;
  memset(&cp, 0, sizeof cp);
  cp.det_boxes = det_boxes; cp.det_count = det_count; cp.masks = masks; cp.n = n; cp.D = D; cp.h = tile_h; cp.w = tile_w;
  cp.Wb = (tile_w + 7) / 8; cp.rects = crop_rects; cp.offsets = crop_offsets; cp.total = crop_total; cp.data = crop_data;
  return launch_mask_crops(cp, s);
}

int rs_engine::launch_polygons(int n, double rdp_epsilon, hipStream_t s) {
  PolyParams pp = poly;
  pp.masks = masks; pp.rects = crop_rects; pp.det_count = det_count; pp.instances = n * D; pp.D = D; pp.h = tile_h; pp.w = tile_w;
  pp.Wb = (tile_w + 7) / 8; pp.eps = rdp_epsilon;
  pp.edge_cap = rs_debug().poly_edge_cap ? rs_debug().poly_edge_cap : PG_EDGE_CAP;
  pp.vertex_cap = rs_debug().poly_vertex_cap ? rs_debug().poly_vertex_cap : PG_VERTEX_CAP;
  return launch_polygonize(pp, s);
}

int rs_engine::enqueue_crop_table(rs_mask_crops* c, int n, hipStream_t s) {
  RS_HIP(hipMemcpyAsync(c->rects, crop_rects, (size_t)n * D * 16, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(c->offsets, crop_offsets, (size_t)n * D * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(h_crop_total, crop_total, 8, hipMemcpyDeviceToHost, s));
  return RS_OK;
}

// after the header event: the byte count has landed, copy exactly the bytes in use
int rs_engine::enqueue_crop_bytes(rs_mask_crops* c, hipStream_t s) {
  const unsigned long long used = *h_crop_total;
  RS_CHECK(used <= c->capacity, RS_ERR_ARG, "mask crops need %llu bytes, the caller's buffer holds %llu", used, (unsigned long long)c->capacity);
  c->used = used;
  if (used) RS_HIP(hipMemcpyAsync(c->data, crop_data, (size_t)used, hipMemcpyDeviceToHost, s));
  return RS_OK;
}

// ===================================================================================== C ABI
extern "C" {

const char* rs_last_error(void) { return g_err; }
int rs_abi_version(void) { return RS_ABI_VERSION; }

int rs_spec_batched_nms(const rs_spec* spec) {
  RS_CHECK(spec, RS_ERR_ARG, "null argument");
  if (spec->struct_size == RS_SPEC_SIZE_V1) return 0;
  RS_CHECK(spec->struct_size == (int32_t)sizeof(rs_spec), RS_ERR_ARG, "rs_spec size mismatch: caller %d, library %d (or %d without batched_nms)",
           spec->struct_size, (int)sizeof(rs_spec), (int)RS_SPEC_SIZE_V1);
  RS_CHECK(spec->batched_nms == 0 || spec->batched_nms == 1, RS_ERR_ARG, "rs_spec.batched_nms %d (0 = per category, 1 = torchvision's size rule)", spec->batched_nms);
  return spec->batched_nms;
}

}  // extern "C"

// rs_engine_create, or with `for_trainer` the forward engine of an rs_trainer (rs_engine::frozen_fusions_only, ::freeze_at)
int engine_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int max_batch,
                  int tile_h, int tile_w, int tile_c, void* stream, bool for_trainer, rs_engine** out, int freeze_at) {
  RS_CHECK(spec && weights && out, RS_ERR_ARG, "null argument");
  const int nms_mode = rs_spec_batched_nms(spec);     // checks struct_size: the current struct, or the one that ends before batched_nms (mode 0)
  if (nms_mode < 0) return nms_mode;
  RS_CHECK(max_batch >= 1 && tile_h >= 32 && tile_w >= 32, RS_ERR_ARG, "bad batch/tile shape");
  int ndev = 0;
  RS_HIP(hipGetDeviceCount(&ndev));
  RS_CHECK(ndev > 0, RS_ERR_HIP, "no HIP device visible: the engine has no CPU fallback");
  RS_CHECK(device_ordinal >= 0 && device_ordinal < ndev, RS_ERR_ARG, "device %d of %d", device_ordinal, ndev);
  RS_HIP(hipSetDevice(device_ordinal));
  rs_engine* e = new rs_engine();
  memcpy(&e->spec, spec, (size_t)spec->struct_size);     // a caller's block may end before batched_nms
  e->spec.struct_size = (int32_t)sizeof(rs_spec);
  e->spec.batched_nms = nms_mode;
  e->device = device_ordinal;
  e->max_batch = max_batch; e->tile_h = tile_h; e->tile_w = tile_w; e->tile_c = tile_c;
  rs_debug_reload();
  e->use_glds = rs_debug().use_glds;
  e->f32 = spec->precision == 1;
  e->split = spec->precision == 2;
  if (e->f32) e->use_glds = -1;
  if (e->split && (e->use_glds <= 0 || for_trainer)) {
    rs_set_error("precision 2 (split operands) needs LDS-DMA staging and is an inference mode");
    delete e;
    return RS_ERR_UNSUPPORTED;
  }
  e->fuse_shortcut = rs_debug().fuse_shortcut;
  e->fuse_bneck = rs_debug().fuse_bneck;
  e->fuse_stem = rs_debug().fuse_stem;
  e->merge_levels = rs_debug().merge_levels;
  // the training engine differentiates every convolution of res3..res5 / FPN / heads separately and needs every layer output there; the frozen
  // stem and res2 (FREEZE_AT 2, what rs_trainer implements) keep the inference engine's fused stem and fused bottleneck tails
  // (the multi-map launches of the FPN output convolutions and of the RPN 3x3 stay: every map still gets its own output tensor; only the RPN heads
  //  leave the 3x3's epilogue, because the trainer differentiates through the 256-channel rpn_conv maps)
  // (a trainer with FREEZE_AT below 2 differentiates res2 as well, and at 0 the stem: those then run unfused too)
  e->frozen_fusions_only = for_trainer;
  e->freeze_at = for_trainer ? freeze_at : 2;
  e->fwd_split_capable = for_trainer && e->f32;      // the opt-in split forward of the fp32 trainer (rs_trainer_set_fwd_mode)
  e->use_graph = rs_debug().use_graph;   // measured: replay == eager (11.54 ms/step either way), so off by default
  if (stream) { e->stream = (hipStream_t)stream; e->own_stream = false; }
  else {
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { rs_set_error("hipStreamCreate: %s", hipGetErrorString(he)); delete e; return RS_ERR_HIP; }
    e->own_stream = true;
  }
  int rc = RS_OK;
  if (hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess) { rs_set_error("hipEventCreate failed"); rc = RS_ERR_HIP; }
  if (!rc) rc = e->parse_blob(weights, nbytes);
  if (!rc) rc = e->build();
  if (!rc) rc = e->assign_phases();
  if (rc) { rs_engine_destroy(e); return rc; }
  *out = e;
  return RS_OK;
}

extern "C" {

int rs_engine_create(const rs_spec* spec, const void* weights, size_t nbytes, int device_ordinal, int max_batch,
                     int tile_h, int tile_w, int tile_c, void* stream, rs_engine** out) {
  return engine_create(spec, weights, nbytes, device_ordinal, max_batch, tile_h, tile_w, tile_c, stream, /*for_trainer=*/false, out);
}

void rs_engine_destroy(rs_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->narrow) { (void)hipStreamSynchronize(e->narrow); (void)hipStreamDestroy(e->narrow); }
  if (e->copy_stream) { (void)hipStreamSynchronize(e->copy_stream); (void)hipStreamDestroy(e->copy_stream); }
  if (e->ev_crop_hdr) (void)hipEventDestroy(e->ev_crop_hdr);
  if (e->h_crop_total) (void)hipHostFree(e->h_crop_total);
  if (e->ev_poly_hdr) (void)hipEventDestroy(e->ev_poly_hdr);
  if (e->h_poly_totals) (void)hipHostFree(e->h_poly_totals);
  if (e->ev_eval_upload) (void)hipEventDestroy(e->ev_eval_upload);
  if (e->ev_band_tiles) (void)hipEventDestroy(e->ev_band_tiles);
  if (e->eval_pinned) (void)hipHostFree(e->eval_pinned);
  if (e->match_pinned) (void)hipHostFree(e->match_pinned);
  if (e->h_sat_copy) (void)hipHostFree(e->h_sat_copy);
  if (e->ev_results) (void)hipEventDestroy(e->ev_results);
  if (e->ev_copied) (void)hipEventDestroy(e->ev_copied);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  for (Stage& st : e->stages) if (st.handoff) (void)hipEventDestroy(st.handoff);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->blob_dev) (void)hipFree(e->blob_dev);
  for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
  for (auto& pr : e->ev_pool) { if (pr.first) (void)hipEventDestroy(pr.first); if (pr.second) (void)hipEventDestroy(pr.second); }
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int rs_engine_infer_device(rs_engine* e, const uint8_t* tiles_dev, int n) {
  RS_CHECK(e && tiles_dev, RS_ERR_ARG, "null argument");
  RS_HIP(hipSetDevice(e->device));
  return e->run(tiles_dev, n);
}

int rs_engine_infer_phase(rs_engine* e, const uint8_t* tiles_dev, int n, int phase) {
  RS_CHECK(e && tiles_dev, RS_ERR_ARG, "null argument");
  RS_CHECK(phase >= 0 && phase < RS_NUM_PHASES, RS_ERR_ARG, "phase %d outside [0, %d)", phase, RS_NUM_PHASES);
  RS_HIP(hipSetDevice(e->device));
  return e->run(tiles_dev, n, phase);
}
int rs_engine_phase_count(void) { return RS_NUM_PHASES; }

// Diagnostic: enqueue, on the engine's wide stream, only the stages whose name contains `substr` (in list order, on the data the last forward left).
int rs_debug_run_stages_matching(rs_engine* e, const char* substr, int n) {
  RS_CHECK(e && substr && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  RS_HIP(hipSetDevice(e->device));
  for (Stage& st : e->stages)
    if (st.name.find(substr) != std::string::npos) {
      int rc = st.fn(n, e->stream);
      if (rc) return rc;
    }
  return RS_OK;
}

int rs_engine_sync(rs_engine* e) {
  RS_CHECK(e, RS_ERR_ARG, "null engine");
  RS_HIP(hipStreamSynchronize(e->stream));
  if (e->narrow) RS_HIP(hipStreamSynchronize(e->narrow));
  return RS_OK;
}

int rs_engine_fetch(rs_engine* e, int n, rs_dets* o) {
  RS_CHECK(e && o && o->count, RS_ERR_ARG, "null argument");
  RS_CHECK(n >= 1 && n <= e->max_batch, RS_ERR_ARG, "batch %d", n);
  RS_CHECK(!o->masks || e->masks, RS_ERR_ARG, "masks requested but MASK_ON is false");
  RS_CHECK(!o->mask_probs || e->mask_probs, RS_ERR_ARG, "mask_probs requested but MASK_ON is false");
  hipStream_t s = e->stream;
  int rc;
  if ((rc = e->enqueue_dets(o, n, s, true))) return rc;
  if (o->mask_probs) RS_HIP(hipMemcpyAsync(o->mask_probs, e->mask_probs, (size_t)n * e->D * RS_MASK_SIDE * RS_MASK_SIDE * 4, hipMemcpyDeviceToHost, s));
  if ((rc = e->sat_copy(s))) return rc;
  RS_HIP(hipStreamSynchronize(s));
  e->sat_publish();
  return RS_OK;
}

// ---- asynchronous host interface: pinned buffers, H2D on the forward stream, D2H on a copy stream behind an event
void* rs_host_alloc(size_t nbytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, nbytes ? nbytes : 16, hipHostMallocDefault) != hipSuccess) { rs_set_error("hipHostMalloc(%zu) failed", nbytes); return nullptr; }
  return p;
}
void rs_host_free(void* p) { if (p) (void)hipHostFree(p); }

// Pin an existing host allocation (the CLI's shared-memory slab of decoded tiles) so that rs_engine_upload_async can copy straight out
// of it: a pageable source makes hipMemcpyAsync stage the bytes through the runtime on the calling thread.
int rs_host_register(void* p, size_t bytes) {
  RS_CHECK(p && bytes > 0, RS_ERR_ARG, "bad argument");
  RS_HIP(hipHostRegister(p, bytes, hipHostRegisterDefault));
  return RS_OK;
}
int rs_host_unregister(void* p) {
  RS_CHECK(p, RS_ERR_ARG, "bad argument");
  RS_HIP(hipHostUnregister(p));
  return RS_OK;
}

int rs_engine_upload_async(rs_engine* e, const uint8_t* tiles_host, int n) {
  RS_CHECK(e && tiles_host && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  { int rc = e->wait_band_tiles(); if (rc) return rc; }
  RS_HIP(hipMemcpyAsync(e->tiles_dev, tiles_host, (size_t)n * e->tile_h * e->tile_w * e->tile_c, hipMemcpyHostToDevice, e->stream));
  return RS_OK;
}

// The asynchronous fetches are sequences of the rs_engine fetch steps above (engine_internal.h).  On the copy stream, in this order:
// crop kernel, polygon kernel, detection copies, crop table, polygon headers, saturation snapshot, ev_copied, the header event.
int rs_engine_fetch_async(rs_engine* e, int n, rs_dets* o) {
  RS_CHECK(e && o && o->count && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->enqueue_dets(o, n, s, true))) return rc;
  return e->end_fetch(s, nullptr);
}

int rs_engine_fetch_crops_async(rs_engine* e, int n, rs_dets* o, rs_mask_crops* c) {
  RS_CHECK(e && o && o->count && c && c->rects && c->offsets && c->data && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  RS_CHECK(e->masks && e->crop_data, RS_ERR_ARG, "mask crops requested but MASK_ON is false");
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_crop_header())) return rc;
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_crops(n, s))) return rc;
  if ((rc = e->enqueue_dets(o, n, s, false))) return rc;
  if ((rc = e->enqueue_crop_table(c, n, s))) return rc;
  return e->end_fetch(s, e->ev_crop_hdr);     // detections and canvases are free for the next forward: the crops live in their own buffer
}

int rs_engine_fetch_crops_wait(rs_engine* e, rs_mask_crops* c) {
  RS_CHECK(e && c && c->data && e->ev_crop_hdr, RS_ERR_ARG, "rs_engine_fetch_crops_wait without rs_engine_fetch_crops_async");
  RS_HIP(hipEventSynchronize(e->ev_crop_hdr));
  { int rc = e->enqueue_crop_bytes(c, e->copy_stream); if (rc) return rc; }
  RS_HIP(hipStreamSynchronize(e->copy_stream));
  e->sat_publish();
  return RS_OK;
}

int rs_engine_fetch_polygons_async(rs_engine* e, int n, rs_dets* o, rs_polygons* g, double rdp_epsilon) {
  RS_CHECK(e && o && o->count && g && g->header && g->poly_ring_count && g->ring_len && g->xy && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  rs_mask_crops* c = g->crops;
  RS_CHECK(c && c->rects && c->offsets && c->data, RS_ERR_ARG, "rs_polygons.crops is incomplete");
  RS_CHECK(e->masks && e->crop_data, RS_ERR_ARG, "polygons requested but MASK_ON is false");
  RS_CHECK(e->tile_h <= PG_MAX_SIDE && e->tile_w <= PG_MAX_SIDE, RS_ERR_UNSUPPORTED, "polygons on the device need tiles up to %d x %d", PG_MAX_SIDE, PG_MAX_SIDE);
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_crop_header())) return rc;
  if ((rc = e->ensure_polygon_buffers())) return rc;
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_crops(n, s))) return rc;
  if ((rc = e->launch_polygons(n, rdp_epsilon, s))) return rc;
  e->poly_forward = e->forward_index; e->poly_tiles = n;      // what rs_engine_fetch_votes_poly_async may read
  if ((rc = e->enqueue_dets(o, n, s, false))) return rc;
  if ((rc = e->enqueue_crop_table(c, n, s))) return rc;
  RS_HIP(hipMemcpyAsync(g->header, e->poly.header, (size_t)n * e->D * PG_HDR * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(e->h_poly_totals, e->poly.totals, 16, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, e->ev_poly_hdr);     // ... and so are they here: crops and polygons live in their own buffers
}

int rs_engine_fetch_polygons_wait(rs_engine* e, rs_polygons* g) {
  RS_CHECK(e && g && g->crops && g->crops->data && e->ev_poly_hdr, RS_ERR_ARG, "rs_engine_fetch_polygons_wait without rs_engine_fetch_polygons_async");
  RS_HIP(hipEventSynchronize(e->ev_poly_hdr));
  const int* t = e->h_poly_totals;
  RS_CHECK((uint64_t)t[0] <= g->poly_cap && (uint64_t)t[1] <= g->ring_cap && (uint64_t)t[2] <= g->vertex_cap, RS_ERR_ARG,
           "polygons need %d / %d / %d rows, the caller's buffers hold %llu / %llu / %llu", t[0], t[1], t[2], (unsigned long long)g->poly_cap,
           (unsigned long long)g->ring_cap, (unsigned long long)g->vertex_cap);
  g->n_polygons = (uint64_t)t[0]; g->n_rings = (uint64_t)t[1]; g->n_vertices = (uint64_t)t[2]; g->n_flagged = (uint64_t)t[3];
  hipStream_t s = e->copy_stream;
  if (t[0]) RS_HIP(hipMemcpyAsync(g->poly_ring_count, e->poly.poly_ring_count, (size_t)t[0] * 4, hipMemcpyDeviceToHost, s));
  if (t[1]) RS_HIP(hipMemcpyAsync(g->ring_len, e->poly.ring_len, (size_t)t[1] * 4, hipMemcpyDeviceToHost, s));
  if (t[2]) RS_HIP(hipMemcpyAsync(g->xy, e->poly.xy, (size_t)t[2] * 4, hipMemcpyDeviceToHost, s));
  g->masks_copied = 0;
  g->crops->used = 0;
  if (t[3] > 0 || g->want_masks) {
    int rc = e->enqueue_crop_bytes(g->crops, s);
    if (rc) return rc;
    g->masks_copied = 1;
  }
  RS_HIP(hipStreamSynchronize(s));
  e->sat_publish();
  return RS_OK;
}

// Does the batch fit the device pool of the validation counts?  RS_OK, RS_EVAL_DOES_NOT_FIT, or an error for tables that are malformed.
int rs_engine_eval_fits(rs_engine* e, int n, const int64_t* poly_off, const int32_t* poly_len, const int32_t* inst_first, const int32_t* tile_first) {
  RS_CHECK(e && inst_first && tile_first && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  RS_CHECK(tile_first[0] == 0, RS_ERR_ARG, "tile_first must start at 0");
  for (int i = 0; i < n; ++i) RS_CHECK(tile_first[i + 1] >= tile_first[i], RS_ERR_ARG, "tile_first decreases at tile %d", i);
  if (!e->masks || e->tile_h != e->tile_w || e->tile_h > CR_MAX_SIDE || ((long long)e->tile_h * ((e->tile_w + 7) / 8)) % 4) return RS_EVAL_DOES_NOT_FIT;
  for (int i = 0; i < n; ++i) if (tile_first[i + 1] - tile_first[i] > RS_EVAL_GT_CAP) return RS_EVAL_DOES_NOT_FIT;
  const int n_inst = tile_first[n];
  RS_CHECK(inst_first[0] == 0, RS_ERR_ARG, "polygons: inst_first must start at 0");
  for (int g = 0; g < n_inst; ++g) RS_CHECK(inst_first[g + 1] >= inst_first[g], RS_ERR_ARG, "polygons: inst_first decreases at instance %d", g);
  const int n_poly = inst_first[n_inst];
  if (n_poly > e->max_batch * 512) return RS_EVAL_DOES_NOT_FIT;
  RS_CHECK(n_poly == 0 || poly_len, RS_ERR_ARG, "polygons: null table");
  size_t doubles = 0;
  for (int q = 0; q < n_poly; ++q) {
    RS_CHECK(poly_len[q] >= 2 && !(poly_len[q] & 1), RS_ERR_ARG, "polygon %d: %d doubles", q, poly_len[q]);
    doubles += (size_t)poly_len[q];
  }
  (void)poly_off;
  return doubles > (size_t)e->max_batch * 65536 ? RS_EVAL_DOES_NOT_FIT : RS_OK;
}

int rs_engine_fetch_eval_async(rs_engine* e, int n, rs_dets* o, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                               const int32_t* inst_first, const int32_t* tile_first, rs_eval_counts* c) {
  RS_CHECK(e && o && o->count && c && c->inter && c->det_area && c->gt_area && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "bad argument");
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, tile_first[n], n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "validation polygons: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_eval_counts(n, &L, s))) return rc;
  if ((rc = e->enqueue_dets(o, n, s, false))) return rc;
  RS_HIP(hipMemcpyAsync(c->inter, e->eval_inter, (size_t)n * e->D * RS_EVAL_GT_CAP * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(c->det_area, e->eval_det_area, (size_t)n * e->D * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(c->gt_area, e->eval_gt_area, (size_t)n * RS_EVAL_GT_CAP * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the counts live in their own buffers: detections and canvases are free for the next forward
}

int rs_engine_fetch_eval_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

// The counts' fetch, then COCOeval's evaluateImg on them (coco_match.h): only detections and match tables travel.
int rs_engine_fetch_eval_match_async(rs_engine* e, int n, rs_dets* o, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                     const int32_t* inst_first, const int32_t* tile_first, const double* gt_boxes, const int32_t* gt_classes,
                                     const double* iou_thrs, rs_eval_matches* m) {
  RS_CHECK(e && o && o->count && m && m->order && m->class_first && m->gt_per_class && m->matched && m->ignored && m->npig && iou_thrs &&
           n >= 1 && n <= e->max_batch, RS_ERR_ARG, "rs_engine_fetch_eval_match_async: bad argument");
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  if (e->D > CM_MAX_SLOTS) return RS_EVAL_DOES_NOT_FIT;
  const int n_inst = tile_first[n], K = e->spec.num_classes, D = e->D, W = (D + 31) / 32;
  RS_CHECK(n_inst == 0 || (gt_boxes && gt_classes), RS_ERR_ARG, "rs_engine_fetch_eval_match_async: null ground-truth boxes or classes");
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, n_inst, n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  if ((rc = e->ensure_match_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "validation polygons: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  const size_t cap = (size_t)e->max_batch * RS_EVAL_GT_CAP;          // n_inst <= n * RS_EVAL_GT_CAP <= cap: rs_engine_eval_fits
  if (n_inst) {
    memcpy(e->match_pinned, gt_boxes, (size_t)n_inst * 32);
    memcpy(e->match_pinned + cap * 32, gt_classes, (size_t)n_inst * 4);
  }
  if ((rc = e->begin_fetch(&s))) return rc;
  if (n_inst) {     // in front of the pool's upload: the event recorded behind that one frees both stagings
    RS_HIP(hipMemcpyAsync(e->match_gt_boxes, e->match_pinned, (size_t)n_inst * 32, hipMemcpyHostToDevice, s));
    RS_HIP(hipMemcpyAsync((uint8_t*)e->match_gt_boxes + cap * 32, e->match_pinned + cap * 32, (size_t)n_inst * 4, hipMemcpyHostToDevice, s));
  }
  if ((rc = e->launch_eval_counts(n, &L, s))) return rc;
  CocoMatchParams q;
  memset(&q, 0, sizeof q);
  q.det_boxes = e->det_boxes; q.det_scores = e->det_scores; q.det_classes = e->det_classes; q.det_count = e->det_count;
  q.gt_boxes = e->match_gt_boxes; q.gt_classes = (const int*)((const uint8_t*)e->match_gt_boxes + cap * 32); q.tile_first = (const int*)e->eval_pool;
  q.inter = e->eval_inter; q.det_area = e->eval_det_area; q.gt_area = e->eval_gt_area;
  q.order = e->match_order; q.class_first = e->match_class_first; q.gt_per_class = e->match_gt_per_class;
  q.matched = e->match_matched; q.ignored = e->match_ignored; q.npig = e->match_npig;
  for (int i = 0; i < CM_THRS; ++i) q.thrs[i] = iou_thrs[i];
  q.n = n; q.K = K; q.D = D; q.g_cap = RS_EVAL_GT_CAP;
  if ((rc = launch_coco_match(q, s))) return rc;
  if ((rc = e->enqueue_dets(o, n, s, false))) return rc;
  const size_t flags = (size_t)n * CM_KINDS * CM_RANGES * CM_THRS * W * 4;
  RS_HIP(hipMemcpyAsync(m->order, e->match_order, (size_t)n * D * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(m->class_first, e->match_class_first, (size_t)n * (K + 1) * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(m->gt_per_class, e->match_gt_per_class, (size_t)n * K * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(m->matched, e->match_matched, flags, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(m->ignored, e->match_ignored, flags, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(m->npig, e->match_npig, (size_t)n * CM_KINDS * CM_RANGES * K * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the tables live in their own buffers: detections and canvases are free for the next forward
}

int rs_engine_fetch_eval_match_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

// The counts of the road labels against the last forward's masks, then the cover vote on them (road_vote.h): only the vote tables and
// the labels' areas travel.  An add-on behind whatever fetch of this forward is already on the copy stream: it copies no detections.
int rs_engine_fetch_votes_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                const int32_t* inst_first, const int32_t* tile_first, double threshold, rs_road_votes* v) {
  RS_CHECK(e && v && v->wscore && v->wfrac && v->pairs && v->label_area && n >= 1 && n <= e->max_batch, RS_ERR_ARG,
           "rs_engine_fetch_votes_async: bad argument");
  RS_CHECK(threshold - threshold == 0.0, RS_ERR_ARG, "rs_engine_fetch_votes_async: the threshold is not finite");
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  if (e->D > RV_MAX_SLOTS) return RS_EVAL_DOES_NOT_FIT;
  const int K = e->spec.num_classes;
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, tile_first[n], n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  if ((rc = e->ensure_vote_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "road labels: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_eval_counts(n, &L, s))) return rc;
  RoadVoteParams q;
  memset(&q, 0, sizeof q);
  q.det_scores = e->det_scores; q.det_classes = e->det_classes; q.det_count = e->det_count; q.tile_first = (const int*)e->eval_pool;
  q.inter = e->eval_inter; q.gt_area = e->eval_gt_area; q.wscore = e->vote_wscore; q.wfrac = e->vote_wscore + e->vote_cells;
  q.pairs = e->vote_pairs; q.threshold = threshold; q.n = n; q.K = K; q.D = e->D; q.g_cap = RS_EVAL_GT_CAP;
  if ((rc = launch_road_votes(q, s))) return rc;
  const size_t cells = (size_t)n * RS_EVAL_GT_CAP * K;
  RS_HIP(hipMemcpyAsync(v->wscore, q.wscore, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->wfrac, q.wfrac, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->pairs, q.pairs, cells * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->label_area, e->eval_gt_area, (size_t)n * RS_EVAL_GT_CAP * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the tables live in their own buffers: detections and canvases are free for the next forward
}

int rs_engine_fetch_votes_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

// The same add-on for a list of thresholds (road_vote.h, THE SWEEP): one upload, one rasteriser pass and one pair count for all of them.
int rs_engine_fetch_vote_sweep_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                     const int32_t* inst_first, const int32_t* tile_first, const double* thresholds, int n_thresholds,
                                     rs_road_vote_sweep* v) {
  RS_CHECK(e && v && v->wscore && v->wfrac && v->pairs && v->label_area && n >= 1 && n <= e->max_batch, RS_ERR_ARG,
           "rs_engine_fetch_vote_sweep_async: bad argument");
  RS_CHECK(thresholds && n_thresholds >= 1 && n_thresholds <= RS_VOTE_SWEEP_MAX, RS_ERR_ARG,
           "rs_engine_fetch_vote_sweep_async: %d thresholds outside [1, %d], or a null list", n_thresholds, RS_VOTE_SWEEP_MAX);
  for (int j = 0; j < n_thresholds; ++j)
    RS_CHECK(thresholds[j] - thresholds[j] == 0.0, RS_ERR_ARG, "rs_engine_fetch_vote_sweep_async: threshold %d is not finite", j);
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  if (e->D > RV_MAX_SLOTS) return RS_EVAL_DOES_NOT_FIT;
  const int K = e->spec.num_classes, T = n_thresholds;
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, tile_first[n], n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  if ((rc = e->ensure_vote_sweep_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "road labels: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_eval_counts(n, &L, s))) return rc;
  RoadVoteSweepParams q;
  memset(&q, 0, sizeof q);
  q.det_scores = e->det_scores; q.det_classes = e->det_classes; q.det_count = e->det_count; q.tile_first = (const int*)e->eval_pool;
  q.inter = e->eval_inter; q.gt_area = e->eval_gt_area; q.wscore = e->sweep_wscore; q.wfrac = e->sweep_wscore + e->sweep_cells;
  q.pairs = e->sweep_pairs; q.T = T; q.n = n; q.K = K; q.D = e->D; q.g_cap = RS_EVAL_GT_CAP;
  for (int j = 0; j < T; ++j) q.thresholds[j] = thresholds[j];
  if ((rc = launch_road_votes_sweep(q, s))) return rc;
  const size_t cells = (size_t)n * T * RS_EVAL_GT_CAP * K;           // <= sweep_cells: n <= max_batch, T <= RS_VOTE_SWEEP_MAX
  RS_HIP(hipMemcpyAsync(v->wscore, q.wscore, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->wfrac, q.wfrac, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->pairs, q.pairs, cells * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->label_area, e->eval_gt_area, (size_t)n * RS_EVAL_GT_CAP * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the tables live in their own buffers: detections and canvases are free for the next forward
}

int rs_engine_fetch_vote_sweep_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

// The vote on polygon areas (poly_overlap.h): the labels' rings against the vertex tables that rs_engine_fetch_polygons_async of THIS
// forward left on the device.  An add-on like the sweep, but neither the rasteriser nor the pair counts run: label upload, overlap
// kernel, the area sweep and five small copies.  The sweep's device tables are shared with rs_engine_fetch_vote_sweep_async (both
// copy them out behind their own kernel on the one copy stream).
int rs_engine_fetch_votes_poly_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                     const int32_t* inst_first, const int32_t* tile_first, const double* thresholds, int n_thresholds,
                                     rs_road_votes_poly* v) {
  RS_CHECK(e && v && v->wscore && v->wfrac && v->pairs && v->label_area && v->flagged && n >= 1 && n <= e->max_batch, RS_ERR_ARG,
           "rs_engine_fetch_votes_poly_async: bad argument");
  RS_CHECK(thresholds && n_thresholds >= 1 && n_thresholds <= RS_VOTE_SWEEP_MAX, RS_ERR_ARG,
           "rs_engine_fetch_votes_poly_async: %d thresholds outside [1, %d], or a null list", n_thresholds, RS_VOTE_SWEEP_MAX);
  for (int j = 0; j < n_thresholds; ++j)
    RS_CHECK(thresholds[j] - thresholds[j] == 0.0, RS_ERR_ARG, "rs_engine_fetch_votes_poly_async: threshold %d is not finite", j);
  RS_CHECK(e->poly_ready && e->poly_forward == e->forward_index && e->poly_tiles == n, RS_ERR_ARG,
           "rs_engine_fetch_votes_poly_async must follow rs_engine_fetch_polygons_async of the same forward and batch");
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  if (e->D > RV_MAX_SLOTS) return RS_EVAL_DOES_NOT_FIT;
  const int K = e->spec.num_classes, T = n_thresholds;
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, tile_first[n], n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  if ((rc = e->ensure_vote_sweep_buffers())) return rc;
  if ((rc = e->ensure_poly_vote_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "road labels: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  if ((rc = e->begin_fetch(&s))) return rc;
  RS_HIP(hipMemcpyAsync(e->eval_pool, e->eval_pinned, L.bytes, hipMemcpyHostToDevice, s));
  RS_HIP(hipEventRecord(e->ev_eval_upload, s));
  e->eval_upload_pending = true;
  PolyOverlapParams o;
  memset(&o, 0, sizeof o);
  o.header = e->poly.header; o.poly_ring_count = e->poly.poly_ring_count; o.ring_len = e->poly.ring_len; o.xy = (const int16_t*)e->poly.xy;
  o.det_count = e->det_count; o.tile_first = (const int*)e->eval_pool; o.inst_first = (const int*)(e->eval_pool + L.o_inst);
  o.poly_off = (const int*)(e->eval_pool + L.o_off); o.poly_len = (const int*)(e->eval_pool + L.o_len); o.polys = (const double*)(e->eval_pool + L.o_xy);
  o.frac = e->pvote_frac; o.label_area = e->pvote_area; o.flagged = e->pvote_flagged; o.n = n; o.D = e->D; o.g_cap = RS_EVAL_GT_CAP;
  if ((rc = launch_poly_overlaps(o, s))) return rc;
  RoadVoteAreaSweepParams q;
  memset(&q, 0, sizeof q);
  q.det_scores = e->det_scores; q.det_classes = e->det_classes; q.det_count = e->det_count; q.tile_first = (const int*)e->eval_pool;
  q.frac = e->pvote_frac; q.wscore = e->sweep_wscore; q.wfrac = e->sweep_wscore + e->sweep_cells; q.pairs = e->sweep_pairs;
  q.T = T; q.n = n; q.K = K; q.D = e->D; q.g_cap = RS_EVAL_GT_CAP;
  for (int j = 0; j < T; ++j) q.thresholds[j] = thresholds[j];
  if ((rc = launch_road_votes_area_sweep(q, s))) return rc;
  const size_t cells = (size_t)n * T * RS_EVAL_GT_CAP * K;           // <= sweep_cells: n <= max_batch, T <= RS_VOTE_SWEEP_MAX
  RS_HIP(hipMemcpyAsync(v->wscore, q.wscore, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->wfrac, q.wfrac, cells * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->pairs, q.pairs, cells * 4, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->label_area, e->pvote_area, (size_t)n * RS_EVAL_GT_CAP * 8, hipMemcpyDeviceToHost, s));
  RS_HIP(hipMemcpyAsync(v->flagged, e->pvote_flagged, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the tables live in their own buffers: detections and vertex tables are free for the next forward
}

int rs_engine_fetch_votes_poly_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

// The band histograms of the road labels under the last forward's tiles (band_hist.h): upload, rasteriser, histogram kernel, one copy.
// An add-on like the vote: no detections, no pair counts.  The kernel is the one reader of tiles_dev on the copy stream: the event
// behind it holds back the next write into the buffer (wait_band_tiles).
int rs_engine_fetch_band_hist_async(rs_engine* e, int n, const double* polys, const int64_t* poly_off, const int32_t* poly_len,
                                    const int32_t* inst_first, const int32_t* tile_first, rs_band_hist* o) {
  RS_CHECK(e && o && o->hist && n >= 1 && n <= e->max_batch, RS_ERR_ARG, "rs_engine_fetch_band_hist_async: bad argument");
  { int rc = rs_engine_eval_fits(e, n, poly_off, poly_len, inst_first, tile_first); if (rc) return rc; }
  RS_CHECK(e->tile_c >= 1 && e->tile_c <= BH_MAX_CHANNELS, RS_ERR_UNSUPPORTED, "rs_engine_fetch_band_hist_async: %d tile channels, the stage holds %d",
           e->tile_c, BH_MAX_CHANNELS);
  MtLayout L;
  { int rc = mt_measure(polys, poly_off, poly_len, inst_first, tile_first[n], n, &L); if (rc) return rc; }
  hipStream_t s = nullptr;
  int rc;
  if ((rc = e->ensure_eval_buffers())) return rc;
  if ((rc = e->ensure_band_buffers())) return rc;
  RS_CHECK(L.bytes <= e->eval_pool_bytes, RS_ERR_ARG, "road labels: %zu bytes packed, the pool holds %zu", L.bytes, e->eval_pool_bytes);
  if (e->eval_upload_pending) { RS_HIP(hipEventSynchronize(e->ev_eval_upload)); e->eval_upload_pending = false; }
  mt_pack(e->eval_pinned, L, polys, poly_off, poly_len, inst_first, tile_first);
  if ((rc = e->begin_fetch(&s))) return rc;
  if ((rc = e->launch_eval_labels(&L, s))) return rc;
  BandHistParams q;
  memset(&q, 0, sizeof q);
  q.tiles = e->tiles_dev; q.label_masks = e->eval_gt_masks; q.tile_first = (const int*)e->eval_pool; q.hist = e->band_hist_dev;
  q.n = n; q.n_inst = tile_first[n]; q.side = e->tile_h; q.C = e->tile_c;
  if ((rc = launch_band_hist(q, s))) return rc;
  RS_HIP(hipEventRecord(e->ev_band_tiles, s));
  e->band_tiles_pending = true;
  if (q.n_inst) RS_HIP(hipMemcpyAsync(o->hist, e->band_hist_dev, (size_t)q.n_inst * q.C * BH_BINS * 4, hipMemcpyDeviceToHost, s));
  return e->end_fetch(s, nullptr);            // the histograms live in a buffer of their own
}

int rs_engine_fetch_band_hist_wait(rs_engine* e) { return rs_engine_fetch_wait(e); }

int rs_engine_fetch_wait(rs_engine* e) {
  RS_CHECK(e, RS_ERR_ARG, "null engine");
  if (e->copy_stream) RS_HIP(hipStreamSynchronize(e->copy_stream));
  e->band_tiles_pending = false;              // the histogram kernel has run: tiles_dev is free
  e->sat_publish();
  return RS_OK;
}

int rs_engine_infer(rs_engine* e, const uint8_t* tiles_host, int n, rs_dets* out_host) {
  RS_CHECK(e && tiles_host && out_host, RS_ERR_ARG, "null argument");
  RS_CHECK(n >= 1 && n <= e->max_batch, RS_ERR_ARG, "batch %d outside [1, %d]", n, e->max_batch);
  RS_HIP(hipSetDevice(e->device));
  { int rc = e->wait_band_tiles(); if (rc) return rc; }
  RS_HIP(hipMemcpyAsync(e->tiles_dev, tiles_host, (size_t)n * e->tile_h * e->tile_w * e->tile_c, hipMemcpyHostToDevice, e->stream));
  int rc = e->run(e->tiles_dev, n);
  if (rc) return rc;
  return rs_engine_fetch(e, n, out_host);
}

void* rs_engine_stream(rs_engine* e) { return e ? (void*)e->stream : nullptr; }

int rs_engine_set_profiling(rs_engine* e, int enabled) {
  RS_CHECK(e, RS_ERR_ARG, "null engine");
  RS_CHECK(enabled >= 0 && enabled <= 3, RS_ERR_ARG, "profiling mode %d", enabled);
  if (e->ev_used) { int rc = e->resolve_profile(); if (rc) return rc; }
  e->forward_index = 0;
  e->poly_forward = -1;
  e->ev_used = 0;
  e->profiling = enabled;
  for (Stage& s : e->stages) { s.ms_total = 0; s.calls = 0; }
  if (enabled >= 2 && e->ev_pool.empty()) {
    const size_t want = e->stages.size() * 32;   // 32 forwards' worth of event pairs
    e->ev_pool.resize(want);
    e->ev_stage.resize(want);
    e->ev_batch.resize(want);
    for (auto& pr : e->ev_pool) {
      RS_HIP(hipEventCreate(&pr.first));
      RS_HIP(hipEventCreate(&pr.second));
    }
  }
  return RS_OK;
}
int rs_engine_stage_count(rs_engine* e) { return e ? (int)e->stages.size() : 0; }
int rs_engine_saturation(rs_engine* e, int64_t* counts, int cap) {
  RS_CHECK(e && (counts || cap <= 0), RS_ERR_ARG, "null argument");
  const int n = (int)e->stages.size();
  for (int i = 0; i < n && i < cap; ++i) counts[i] = i < (int)e->h_sat.size() ? e->h_sat[i] : 0;
  return n;
}
int rs_engine_stage_info(rs_engine* e, int i, char* name_out, double* ms_total, int* calls, double* flops, double* bytes) {
  RS_CHECK(e && i >= 0 && i < (int)e->stages.size(), RS_ERR_ARG, "stage index");
  if (e->ev_used) { int rc = e->resolve_profile(); if (rc) return rc; }
  const Stage& s = e->stages[i];
  if (name_out) { strncpy(name_out, s.name.c_str(), 95); name_out[95] = 0; }
  if (ms_total) *ms_total = s.ms_total;
  if (calls) *calls = s.calls;
  if (flops) *flops = s.last_flops;
  if (bytes) *bytes = s.last_bytes;
  return RS_OK;
}

int rs_engine_stage_kernel(rs_engine* e, int i, char* name_out) {
  RS_CHECK(e && i >= 0 && i < (int)e->stages.size() && name_out, RS_ERR_ARG, "stage index");
  static const char* names[] = {"conv_igemm_kernel<2,2,4,4> 128x128", "conv_igemm_kernel<4,1,4,4> 256x64", "conv_igemm_kernel<4,1,1,4> 256x16 f32-out",
                                "conv_igemm_kernel<4,2,4,4> 256x128", "conv_igemm_kernel<2,4,4,8> 256x256", "conv_igemm_kernel<4,1,4,4,smallC> 256x64 stem",
                                "(retired)",
                                "conv_igemm_kernel<2,2,4,2> 64x128", "conv_igemm_kernel<4,1,4,2> 128x64", "conv_igemm_kernel<2,2,4,1> 32x128",
                                "conv_igemm_kernel<2,4,4,2> 64x256", "(retired)",
                                "conv_deep_kernel 256x256 (3 activation + 2 weight LDS stages)",
                                "bneck_tail_kernel 128 px (conv2 + conv3 + next conv1 chained through registers)",
                                "conv_igemm_kernel<2,4,4,4> 128x256",
                                "conv_deep_kernel 160x256", "conv_deep_kernel 192x256", "conv_deep_kernel 224x256",
                                "conv_deep_kernel 64x256", "conv_deep_kernel 96x256", "conv_deep_kernel 128x256",
                                "stem_pool_kernel (conv 7x7 s2 + ReLU + max-pool 3x3 s2, 8x8 pooled pixels per workgroup)",
                                "conv1x1_wreg_kernel 32 px x 256 ch (persistent, weights in registers, operand tiles by LDS-DMA, two workgroups per CU)",
                                "bneck_tail_split_kernel 128 px (conv2 + conv3 + next conv1 chained through registers)"};
  const int v = e->stages[i].variant;
  const char* s = v == -1 ? "conv_f32_mfma_kernel" : (v >= 0 && v <= 23 ? names[v] : (v >= 28 && v <= 31 ? "conv_wide1x1_split_kernel (all rows per pixel tile, pixels in registers)" : ""));
  if (e->split && ((v >= 0 && v <= 23) || (v >= 28 && v <= 31))) {
    snprintf(name_out, 96, "%.62s [split: hi+lo planes, 3 MFMA blocks]", s);
    return RS_OK;
  }
  strncpy(name_out, s, 95);
  name_out[95] = 0;
  return RS_OK;
}

int rs_engine_stage_variant(rs_engine* e, int i) {
  if (!e || i < 0 || i >= (int)e->stages.size()) return -2;
  return e->stages[i].variant;
}

int rs_engine_tensor(rs_engine* e, const char* name, void** dev_ptr, int* dtype, int* ndim, int64_t dims[5], int* halo) {
  RS_CHECK(e && name, RS_ERR_ARG, "null argument");
  for (const TensorInfo& t : e->tensors) {
    if (t.name == name) {
      if (dev_ptr) *dev_ptr = t.p;
      if (dtype) *dtype = t.dtype;
      if (ndim) *ndim = t.ndim;
      if (dims) for (int i = 0; i < 5; ++i) dims[i] = t.dims[i];
      if (halo) *halo = t.halo;
      return RS_OK;
    }
  }
  rs_set_error("no tensor named %s", name);
  return RS_ERR_ARG;
}
int rs_engine_tensor_count(rs_engine* e) { return e ? (int)e->tensors.size() : 0; }
int rs_engine_tensor_name(rs_engine* e, int i, char* name_out) {
  RS_CHECK(e && i >= 0 && i < (int)e->tensors.size() && name_out, RS_ERR_ARG, "tensor index");
  strncpy(name_out, e->tensors[i].name.c_str(), 95);
  name_out[95] = 0;
  return RS_OK;
}

int rs_engine_net_shape(rs_engine* e, int* rh, int* rw, int* ph, int* pw) {
  RS_CHECK(e, RS_ERR_ARG, "null engine");
  if (rh) *rh = e->net_h;
  if (rw) *rw = e->net_w;
  if (ph) *ph = e->pad_h;
  if (pw) *pw = e->pad_w;
  return RS_OK;
}

// rs_op_mask_overlap on the detection masks of tile `tile` of the engine's last forward (all D slots; slots >= count hold stale
// canvases, the caller reads the first count[tile] columns)
int rs_engine_label_overlap(rs_engine* e, int tile, const uint8_t* label_masks_dev, int n_labels, int32_t* inter_dev, int32_t* label_area_dev) {
  RS_CHECK(e && e->masks && tile >= 0 && tile < e->max_batch && label_masks_dev && inter_dev && label_area_dev, RS_ERR_ARG, "bad argument");
  const size_t per = (size_t)e->tile_h * ((e->tile_w + 7) / 8);
  return launch_mask_overlap(e->masks + (size_t)tile * e->D * per, e->D, label_masks_dev, n_labels, e->tile_h, e->tile_w, inter_dev, label_area_dev, e->stream);
}

}  // extern "C"
