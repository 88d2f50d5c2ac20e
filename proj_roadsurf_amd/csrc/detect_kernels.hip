// Proposal / detection "glue" of the Mask R-CNN forward on gfx950: everything between the conv
// GEMMs.  All box and score arithmetic is fp32 in the same operation order as detectron2 0.6 /
// torchvision 0.11.3 (this file is compiled with -ffp-contract=off so no mul+add is fused), all
// index work is exact; capacities are fixed and counts stay on the device (no host sync).
//
//   rpn_select_kernel   RPN.predict_proposals / find_top_rpn_proposals, per (image, level):
//                       radix-select top-k logits (ties: lower anchor index first), bitonic sort,
//                       anchor-free decode (anchors recomputed from the index), clip, non-empty.
//                       [EXT d2: modeling/proposal_generator/{rpn,proposal_utils}.py,
//                        modeling/anchor_generator.py, modeling/box_regression.py]  R:40-56,222-251
//   nms_kernel          torchvision nms (IoU > thr suppresses), one workgroup per (image, level) or
//                       (image, class): 64-bit suppression bitmask in LDS + single-wave scan.
//                       [EXT tv: csrc/ops/cuda/nms_kernel.cu]
//   rpn_merge_kernel    batched_nms result order (score desc) + POST_NMS_TOPK.   R:247
//   (ROIPooler level assignment + ROIAlign: roi_align.hip, over the geometry of roi_geom.h)   R:172-174,219-221
//   box_candidates_kernel / det_merge_kernel   fast_rcnn_inference_single_image + the box part of
//                       detector_postprocess  [EXT d2: modeling/roi_heads/fast_rcnn.py,
//                       modeling/postprocessing.py]  R:160-165,190,194,321
//   mask_predict_kernel mask predictor 1x1 on the predicted class + sigmoid (mask_rcnn_inference)
//   paste_masks_kernel  paste_masks_in_image (grid_sample bilinear, zeros, align_corners=False) >= thr,
//                       bit-packed output  [EXT d2: layers/mask_ops.py]
#include "detect.h"
#include "roi_geom.h"

namespace {

__device__ __forceinline__ uint32_t fkey(float f) {
  f = f + 0.0f;   // -0 -> +0 so that equal floats have equal keys
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// descending bitonic sort of n (power of two) 64-bit keys in LDS
template <int T>
__device__ void bitonic_sort_desc(unsigned long long* s, int n, int tid) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n; i += T) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = s[i], b = s[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (a < b) : (a > b)) { s[i] = b; s[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// smallest power of two >= c inside [lo, hi]: the bitonic sorts of the merge kernels run over the entries that exist (the rest of the list is zero
// keys, which a descending sort leaves where they are), not over the capacity -- 66 passes over 2 048 entries instead of 91 over 8 192 when a tile
// keeps 2 000 candidates; at batch 1 these one-workgroup kernels are a third of the forward's latency
__device__ __forceinline__ int sort_size(unsigned c, int lo, int hi) {
  int n = lo;
  while (n < hi && (unsigned)n < c) n <<= 1;
  return n;
}

// Box2BoxTransform.apply_deltas for one box, one delta quadruple (fp32, detectron2 op order).
__device__ __forceinline__ void apply_deltas(const float b[4], const float d[4], float wx, float wy, float ww, float wh,
                                             float scale_clamp, float out[4]) {
  const float widths = b[2] - b[0];
  const float heights = b[3] - b[1];
  const float ctr_x = b[0] + 0.5f * widths;
  const float ctr_y = b[1] + 0.5f * heights;
  const float dx = rs_fdiv(d[0], wx), dy = rs_fdiv(d[1], wy);
  float dw = rs_fdiv(d[2], ww), dh = rs_fdiv(d[3], wh);
  dw = dw > scale_clamp ? scale_clamp : dw;
  dh = dh > scale_clamp ? scale_clamp : dh;
  const float pcx = dx * widths + ctr_x;
  const float pcy = dy * heights + ctr_y;
  const float pw = expf(dw) * widths;
  const float ph = expf(dh) * heights;
  out[0] = pcx - 0.5f * pw;
  out[1] = pcy - 0.5f * ph;
  out[2] = pcx + 0.5f * pw;
  out[3] = pcy + 0.5f * ph;
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---------------------------------------------------------------------------------------------
// RPN: select + decode
// ---------------------------------------------------------------------------------------------
// CAP = candidate capacity per (image, level): 1024 (inference, PRE_NMS_TOPK_TEST 1000) or 2048 (training, PRE_NMS_TOPK_TRAIN 2000)
template <int CAP>
__global__ __launch_bounds__(1024) void rpn_select_kernel(const RpnParams p) {
  __shared__ unsigned long long list[CAP];
  __shared__ int hist[256];
  __shared__ int hist16[16 * 257];
  __shared__ unsigned int sh_prefix, sh_need, sh_cnt, sh_idx_thr, sh_ccount, sh_tie;
  const int l = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int H = p.H[l], W = p.W[l], A = p.A;
  const int HW = H * W;
  const int n_el = HW * A;
  const int k = n_el < p.topk ? n_el : p.topk;
  const float* head = p.head[l] + (long long)n * HW * p.cs;
  uint32_t* keys = p.keys[l] + (long long)n * 2 * n_el;     // [n_el] ordered keys, then [n_el] candidate indices
  uint32_t* cidx = keys + n_el;

  // Scan A: ordered keys to scratch + histogram of the top 8 bits.
  if (tid < 256) hist[tid] = 0;
  if (tid == 0) { sh_prefix = 0; sh_need = (unsigned)k; sh_cnt = 0; sh_ccount = 0; sh_idx_thr = 0xFFFFFFFFu; }
  for (int i = tid; i < CAP; i += 1024) list[i] = 0ull;
  __syncthreads();
  // Logits share sign and exponent, so the top digit hits a handful of bins: 16 privatised, bank-
  // staggered sub-histograms cut the same-address serialisation of the LDS atomics 16-fold.
  // (wave-aggregated ballot atomics were measured slower: 0.29 vs 0.24 ms)
  for (int i = tid; i < 16 * 257; i += 1024) hist16[i] = 0;
  __syncthreads();
  // 8 independent loads in flight per lane: with one workgroup per (image, level) the scan is bound by
  // load latency, not bandwidth.
  for (int base = 0; base < n_el; base += 8192) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * 1024 + tid;
      const int pix = e / A, a = e - pix * A;
      v[u] = e < n_el ? head[(long long)pix * p.cs + a] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = base + u * 1024 + tid;
      if (e < n_el) {
        const uint32_t key = fkey(v[u]);
        keys[e] = key;
        atomicAdd(&hist16[(tid & 15) * 257 + (key >> 24)], 1);
      }
    }
  }
  __syncthreads();
  if (tid < 256) {
    int sum = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) sum += hist16[q * 257 + tid];
    hist[tid] = sum;
  }
  __syncthreads();
  auto pick_desc = [&](int shift) {     // thread 0: bin holding the need-th largest, walking from the top
    unsigned need = sh_need, acc = 0;
    int b = 255;
    for (; b > 0; --b) {
      if (acc + (unsigned)hist[b] >= need) break;
      acc += (unsigned)hist[b];
    }
    sh_need = need - acc;              // still to take from bin b
    sh_prefix |= ((unsigned)b) << shift;
    sh_tie = (unsigned)hist[b];        // elements in bin b under the current prefix
  };
  if (p.debug == 1) return;
  if (tid == 0) pick_desc(24);
  __syncthreads();
  if (p.debug == 2) return;
  // Scan B: everything above the selected top-digit bin is in; the bin itself (typically ~10 % of the
  // anchors) is compacted to a candidate list, so the remaining digit passes touch only candidates.
  {
    const uint32_t b0 = sh_prefix >> 24;
    for (int base = 0; base < n_el; base += 8192) {
      uint32_t kv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + u * 1024 + tid;
        kv[u] = e < n_el ? keys[e] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + u * 1024 + tid;
        if (e >= n_el) continue;
        const uint32_t key = kv[u];
        const uint32_t top = key >> 24;
        if (top > b0) {
          const unsigned pos = atomicAdd(&sh_cnt, 1u);
          if (pos < (unsigned)CAP) list[pos] = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)e);
        } else if (top == b0) {
          const unsigned c = atomicAdd(&sh_ccount, 1u);
          cidx[c] = (uint32_t)e;
        }
      }
    }
  }
  __syncthreads();
  if (p.debug == 3) return;
  const int nc = (int)sh_ccount;
  for (int d = 1; d < 4; ++d) {
    const int shift = 24 - 8 * d;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = sh_prefix;
    for (int ci = tid; ci < nc; ci += 1024) {
      const uint32_t key = keys[cidx[ci]];
      if ((key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid == 0) pick_desc(shift);
    __syncthreads();
  }
  if (p.debug == 4) return;
  const uint32_t T = sh_prefix;       // k-th largest key
  // ties on the threshold key: take the lowest anchor indices (radix select on the index)
  if (sh_tie > sh_need) {              // uniform
    __syncthreads();
    if (tid == 0) sh_prefix = 0;
    __syncthreads();
    for (int d = 0; d < 3; ++d) {
      const int shift = 16 - 8 * d;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const uint32_t prefix = sh_prefix;
      for (int ci = tid; ci < nc; ci += 1024) {
        const uint32_t e = cidx[ci];
        if (keys[e] == T && (d == 0 || (e >> (shift + 8)) == (prefix >> (shift + 8))))
          atomicAdd(&hist[(e >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned need = sh_need, acc = 0;
        int b = 0;
        for (; b < 255; ++b) {
          if (acc + (unsigned)hist[b] >= need) break;
          acc += (unsigned)hist[b];
        }
        sh_need = need - acc;
        sh_prefix |= ((unsigned)b) << shift;
      }
      __syncthreads();
    }
    if (tid == 0) sh_idx_thr = sh_prefix;   // largest index taken among the ties
    __syncthreads();
  }
  const uint32_t idx_thr = sh_idx_thr;
  for (int ci = tid; ci < nc; ci += 1024) {
    const uint32_t e = cidx[ci];
    const uint32_t key = keys[e];
    if (key > T || (key == T && e <= idx_thr)) {
      const unsigned pos = atomicAdd(&sh_cnt, 1u);
      if (pos < (unsigned)CAP) list[pos] = ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - e);
    }
  }
  __syncthreads();
  if (p.debug == 5) return;
  bitonic_sort_desc<1024>(list, CAP, tid);
  if (p.debug == 6) return;

  const long long ob = ((long long)n * p.L + l) * CAP;
  if (tid == 0) p.cand_count[n * p.L + l] = k;
  for (int ti = tid; ti < k; ti += 1024) {
    const unsigned long long c = list[ti];
    const uint32_t e = 0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull);
    const float score = fkey_inv((uint32_t)(c >> 32));
    const int pix = e / A, a = e - pix * A;
    const int y = pix / W, x = pix - y * W;
    const float sx = (float)(x * p.stride[l]) + p.offset * (float)p.stride[l];
    const float sy = (float)(y * p.stride[l]) + p.offset * (float)p.stride[l];
    float anc[4] = {sx + p.base[l][a][0], sy + p.base[l][a][1], sx + p.base[l][a][2], sy + p.base[l][a][3]};
    const float* dp = head + (long long)pix * p.cs + A + a * 4;
    float d[4] = {dp[0], dp[1], dp[2], dp[3]};
    float b[4];
    apply_deltas(anc, d, p.wx, p.wy, p.ww, p.wh, p.scale_clamp, b);
    const float ih = p.img_hw ? p.img_hw[2 * n] : p.img_h, iw = p.img_hw ? p.img_hw[2 * n + 1] : p.img_w;
    b[0] = clampf(b[0], 0.f, iw);
    b[1] = clampf(b[1], 0.f, ih);
    b[2] = clampf(b[2], 0.f, iw);
    b[3] = clampf(b[3], 0.f, ih);
    float* ob4 = p.cand_boxes + (ob + ti) * 4;
    ob4[0] = b[0]; ob4[1] = b[1]; ob4[2] = b[2]; ob4[3] = b[3];
    p.cand_scores[ob + ti] = score;
    p.cand_valid[ob + ti] = ((b[2] - b[0]) > p.min_size && (b[3] - b[1]) > p.min_size) ? 1 : 0;
    if (p.cand_index) p.cand_index[ob + ti] = (int)e;
  }
}

// ---------------------------------------------------------------------------------------------
// torchvision.ops.batched_nms, the decision per image ([EXT tv: ops/boxes.py], 0.11): with boxes.numel() > 4000 one NMS per category,
// else ONE NMS over boxes + category * (boxes.max() + 1).  A workgroup counts the boxes of its image that enter the call (valid entries of
// all its segments) and, only where the rule is taken, reduces their largest coordinate.  Part of nms_kernel's prologue (NmsParams::rule):
// every workgroup of an image repeats the image's reduction (at most 1000 boxes where it goes beyond the counts), which measured cheaper than
// a launch of its own in front of the NMS.
// Where this is not torch: fmaxf drops a NaN coordinate that boxes.max() would propagate (the RPN's valid flags already exclude non-finite
// boxes; the box head's decoded, clipped boxes are finite unless the network's output is not); and entries beyond the capacity (count > cap)
// are counted but carry no box, so callers keep cap >= 1001 in this mode (launch_nms checks it): the rule then cannot be taken with any such entry.
// ---------------------------------------------------------------------------------------------
// By all 1024 threads of a workgroup (uniform control flow, two barriers): returns rule taken, *total and *unit to every thread.
__device__ __forceinline__ bool nms_rule_decide(const float* boxes, const int* count, const uint8_t* valid, int cap, int group, int img,
                                                int* total_out, float* unit_out) {
  __shared__ int s_cnt[16];
  __shared__ float s_max[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long s0 = (long long)img * group;
  int cnt = 0;
  for (int g = 0; g < group; ++g) {
    int raw = count[s0 + g];
    if (raw < 0) raw = 0;
    const int n = raw < cap ? raw : cap;
    if (!valid) { if (tid == 0) cnt += raw; continue; }
    if (tid == 0) cnt += raw - n;               // the uncapped count decides: entries beyond the capacity carry no flag
    const uint8_t* v = valid + (s0 + g) * cap;
    for (int i = tid; i < n; i += 1024) cnt += v[i] ? 1 : 0;
  }
  for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  int total = 0;
  for (int w = 0; w < 16; ++w) total += s_cnt[w];
  *total_out = total;
  *unit_out = 0.f;
  if (!(total >= 1 && total <= 1000)) return false;    // uniform.  !(boxes.numel() > 4000), and an empty call returns before the rule
  float m = -INFINITY;
  for (int g = 0; g < group; ++g) {
    int n = count[s0 + g];
    if (n > cap) n = cap;
    const float* b4 = boxes + (s0 + g) * cap * 4;
    const uint8_t* v = valid ? valid + (s0 + g) * cap : nullptr;
    for (int i = tid; i < n; i += 1024) {
      if (v && !v[i]) continue;
      const float4 b = *(const float4*)(b4 + (long long)i * 4);
      m = fmaxf(fmaxf(m, fmaxf(b.x, b.y)), fmaxf(b.z, b.w));
    }
  }
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0) s_max[wave] = m;
  __syncthreads();
  for (int w = 0; w < 16; ++w) m = fmaxf(m, s_max[w]);
  *unit_out = m + 1.0f;
  return true;
}

// ---------------------------------------------------------------------------------------------
// NMS over a segment of <= CAP boxes already in priority order.  CAP 1024: the suppression mask (128 KB) lives in LDS;
// CAP 2048 (training, PRE_NMS_TOPK_TRAIN 2000): 512 KB per segment in a global scratch buffer (L2-resident).
// ---------------------------------------------------------------------------------------------
// GM: the suppression mask lives in global memory (NmsParams::scratch) instead of LDS -- needed for CAP 2048, and used for CAP 1024 when few segments
// are launched (batch 1-3): the quadratic mask build is then shared by gridDim.y workgroups (mode 1) and the scan runs as a second launch (mode 2)
template <int CAP, bool GM>
__global__ __launch_bounds__(1024) void nms_kernel(const NmsParams p) {
  constexpr int WPR = CAP / 64;                                       // mask words per row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* sbox = (float4*)smem;                                       // CAP * 16
  float* sarea = (float*)(smem + CAP * 16);                           // CAP * 4
  unsigned long long* sremoved = (unsigned long long*)(smem + CAP * 20);   // WPR * 8
  const int s = blockIdx.x, tid = threadIdx.x;
  unsigned long long* mask = !GM ? (unsigned long long*)(smem + CAP * 20 + 256)
                                 : p.scratch + (long long)s * CAP * WPR;
  int n = p.count[s];
  if (n > CAP) n = CAP;
  const float* boxes = p.boxes + (long long)s * p.cap * 4;
  const uint8_t* valid = p.valid ? p.valid + (long long)s * p.cap : nullptr;
  uint8_t* keep = p.keep + (long long)s * p.cap;
  if (!(GM && p.mode == 1)) for (int i = tid; i < p.cap; i += 1024) keep[i] = 0;
  // An empty segment has nothing to build or scan and its keep flags are zero already: with many classes most segments of a trained
  // detector are empty, and a workgroup that holds 148 KB of LDS should not queue behind them.  Under the size rule the first
  // segment of an image still writes the image's decision out.
  if (n <= 0 && !(p.rule && !(GM && p.mode == 2) && s % p.group == 0 && blockIdx.y == 0)) return;
  if (tid < WPR) sremoved[tid] = 0ull;
  __syncthreads();
  // batched_nms's coordinate offsets (NmsParams::rule): `idxs.to(boxes) * (max_coordinate + 1)` is one rounded product, `boxes + offsets[:, None]`
  // four rounded adds; areas and IoUs then come from the shifted values.  The boxes in memory stay as they are.
  bool shift = false;
  float off = 0.f;
  if (p.rule && !(GM && p.mode == 2)) {         // (the scan launch reads no box)
    const int img = s / p.group, g = s - img * p.group;
    int total;
    float unit;
    shift = nms_rule_decide(p.boxes, p.count, p.valid, p.cap, p.group, img, &total, &unit);
    if (shift) off = (float)g * unit;
    if (g == 0 && blockIdx.y == 0 && tid == 0) { p.rule[2 * img] = shift ? 1 : 0; p.rule[2 * img + 1] = total; p.unit[img] = unit; }
  }
  for (int ti = tid; ti < n; ti += 1024) {
    float4 b = *(const float4*)(boxes + ti * 4);
    if (shift) { b.x = b.x + off; b.y = b.y + off; b.z = b.z + off; b.w = b.w + off; }
    sbox[ti] = b;
    sarea[ti] = (b.z - b.x) * (b.w - b.y);
    if (valid && !valid[ti]) atomicOr(&sremoved[ti >> 6], 1ull << (ti & 63));
  }
  __syncthreads();
  const int nw = (n + 63) >> 6;
  // Row i needs words (i>>6) .. nw-1 only, a triangular amount of work.  Rows are paired (i, n-1-i)
  // so that every task slot (row pair, word slot) carries the same load and all 16 waves stay busy.
  const int nh = (n + 1) >> 1;
  const int nhp = (nh + 63) & ~63;
  const bool build = p.debug != 2 && !(GM && p.mode == 2);
  for (int idx = tid + blockIdx.y * 1024; idx < (nw + 2) * nhp && build; idx += 1024 * gridDim.y) {
    const int wq = idx / nhp, ip = idx - wq * nhp;
    if (ip >= nh) continue;
    const int first = nw - (ip >> 6);
    int i, w;
    if (wq < first) { i = ip; w = (ip >> 6) + wq; }
    else {
      i = n - 1 - ip;
      w = (i >> 6) + (wq - first);
      if (i == ip || w >= nw) continue;
    }
    unsigned long long bits = 0ull;
    const int j0 = w * 64;
    if (j0 + 63 > i) {
      const float4 a = sbox[i];
      const float sa = sarea[i];
      const float thr = p.thresh;
      // torchvision: suppress when fl(inter / (sa + sb - inter)) > thr.  The division is only needed when
      // inter is within 1e-5 (relative) of thr * union; outside that band the comparison of the products
      // decides identically (fp32 rounding is 6e-8), so the result stays bit-exact with the reference.
      auto test = [&](int j) -> bool {
        const float4 q = sbox[j];
        const float iw = fmaxf(fminf(a.z, q.z) - fmaxf(a.x, q.x), 0.f);
        const float ih = fmaxf(fminf(a.w, q.w) - fmaxf(a.y, q.y), 0.f);
        const float inter = iw * ih;
        if (!(inter > 0.f)) return false;           // 0/x = 0, 0/0 = NaN: never > thr
        const float uni = sa + sarea[j] - inter;
        const float tu = thr * uni;
        if (inter > tu * 1.00001f) return true;
        if (!(inter > tu * 0.99999f)) return false;
        return rs_fdiv(inter, uni) > thr;
      };
      unsigned lo = 0u, hi = 0u;
      if (j0 > i && j0 + 64 <= n) {                 // word entirely right of the diagonal and inside n
#pragma unroll 4
        for (int b = 0; b < 32; ++b) if (test(j0 + b)) lo |= 1u << b;
#pragma unroll 4
        for (int b = 0; b < 32; ++b) if (test(j0 + 32 + b)) hi |= 1u << b;
      } else {
        for (int b = 0; b < 32; ++b) { const int j = j0 + b; if (j > i && j < n && test(j)) lo |= 1u << b; }
        for (int b = 0; b < 32; ++b) { const int j = j0 + 32 + b; if (j > i && j < n && test(j)) hi |= 1u << b; }
      }
      bits = ((unsigned long long)hi << 32) | lo;
    }
    mask[(long long)i * WPR + w] = bits;
  }
  if (GM && p.mode == 1) return;                // mask build only: the scan is the next launch (mode 2)
  if (GM) __threadfence();       // mask rows in global memory: visible to the scanning wave after the barrier
  __syncthreads();
  // Greedy scan, one wave, 64 boxes (one mask word) per step: the intra-chunk part is resolved on
  // the scalar unit from the diagonal words (lane b holds row b), then the rows of the survivors
  // are OR-ed into the later words by all 64 lanes in parallel.
  if (tid < 64 && p.debug != 1) {
    const int lane = tid;
    unsigned long long removed = lane < WPR ? sremoved[lane] : 0ull;   // lane w holds word w
    for (int c = 0; c < nw; ++c) {
      const int base = c * 64;
      const int cnt = (n - base) < 64 ? (n - base) : 64;
      const unsigned long long rem_c = __shfl(removed, c);
      const unsigned long long diag = lane < cnt ? mask[(long long)(base + lane) * WPR + c] : 0ull;
      const int dlo = (int)(unsigned)(diag & 0xFFFFFFFFull), dhi = (int)(unsigned)(diag >> 32);
      unsigned long long alive = ~rem_c;
      if (cnt < 64) alive &= (1ull << cnt) - 1ull;
      unsigned alo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(alive & 0xFFFFFFFFull));
      unsigned ahi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(alive >> 32));
      unsigned long long al = ((unsigned long long)ahi << 32) | alo;
      unsigned long long kept = 0ull;
      while (al) {
        const int b = __builtin_ctzll(al);
        kept |= 1ull << b;
        const unsigned rlo = (unsigned)__builtin_amdgcn_readlane(dlo, b);
        const unsigned rhi = (unsigned)__builtin_amdgcn_readlane(dhi, b);
        al &= ~(((unsigned long long)rhi << 32) | rlo);
        al &= ~(1ull << b);
      }
      if (lane < cnt) keep[base + lane] = (uint8_t)((kept >> lane) & 1ull);
      const int w = lane & (WPR - 1);
      unsigned long long part = 0ull;
      if (w > c && w < nw) {
        for (int b = lane / WPR; b < cnt; b += 64 / WPR)
          if ((kept >> b) & 1ull) part |= mask[(long long)(base + b) * WPR + w];
      }
      if (WPR == 16) part |= __shfl_xor(part, 16);
      part |= __shfl_xor(part, 32);
      if (lane < WPR) removed |= part;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// RPN: merge levels (score desc, ties: lower (level, rank) first), keep post_topk
// ---------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(1024) void rpn_merge_kernel(const RpnMergeParams p) {
  constexpr int SORTN = CAP * 8;                          // up to 8 levels' candidates (power of two for the bitonic sort)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* list = (unsigned long long*)smem;   // SORTN
  __shared__ unsigned int cnt;
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  for (int i = tid; i < SORTN; i += 1024) list[i] = 0ull;
  __syncthreads();
  for (int l = 0; l < p.L; ++l) {
    const int c = p.cand_count[n * p.L + l];
    const long long ob = ((long long)n * p.L + l) * CAP;
    for (int i = tid; i < c; i += 1024) {
      if (p.keep[ob + i]) {
        const unsigned pos = atomicAdd(&cnt, 1u);
        list[pos] = ((unsigned long long)fkey(p.cand_scores[ob + i]) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(l * CAP + i));
      }
    }
  }
  __syncthreads();
  bitonic_sort_desc<1024>(list, sort_size(cnt, 1024, SORTN), tid);
  const int total = (int)cnt < p.post_topk ? (int)cnt : p.post_topk;
  if (tid == 0) p.prop_count[n] = total;
  for (int i = tid; i < p.cap; i += 1024) {
    float* o = p.prop_boxes + ((long long)n * p.cap + i) * 4;
    if (i < total) {
      const uint32_t pos = 0xFFFFFFFFu - (uint32_t)(list[i] & 0xFFFFFFFFull);
      const long long src = (long long)n * p.L * CAP + pos;
      const float* b = p.cand_boxes + src * 4;
      o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
      p.prop_scores[(long long)n * p.cap + i] = p.cand_scores[src];
      if (p.prop_level) p.prop_level[(long long)n * p.cap + i] = (int)(pos / CAP);
    } else {
      o[0] = o[1] = o[2] = o[3] = 0.f;
      p.prop_scores[(long long)n * p.cap + i] = 0.f;
    }
  }
  if (!p.prop_order) return;                  // uniform
  // Visiting order of the RoI pooler: the proposals leave this kernel in score order, i.e. scattered over the image; sorted by
  // (pooler level, top row, left column) consecutive workgroups of box.roi_align read neighbouring rows of ONE feature map and hit
  // in L2 (measured HBM bytes of that kernel: 1.77x its algorithmic traffic in score order).  Pure scheduling: every RoI is
  // pooled into its own slot exactly as before.
  __syncthreads();                            // list[] (the score order) has been consumed
  for (int i = tid; i < 1024; i += 1024) {
    unsigned long long key = 0ull;            // descending sort: invalid slots (key 0) come last
    if (i < total && i < p.cap) {
      const float* b = p.prop_boxes + ((long long)n * p.cap + i) * 4;
      const unsigned lvl = (unsigned)roi_level(b[0], b[1], b[2], b[3], 4);   // the pooler's own level (p2..p5)
      unsigned yq = (unsigned)fmaxf(b[1], 0.f), xq = (unsigned)fmaxf(b[0], 0.f);
      yq = yq > 8191u ? 8191u : yq; xq = xq > 8191u ? 8191u : xq;
      const unsigned k32 = (lvl << 26) | (yq << 13) | xq;                 // ascending in (level, y, x) ...
      key = ((unsigned long long)(0xFFFFFFFFu - k32) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i) ;   // ... under a descending sort
      key |= 1ull << 63;                      // valid slots before the zero keys (k32 < 2^28, so bit 63 of ~k32 is set anyway)
    }
    list[i] = key;
  }
  __syncthreads();
  bitonic_sort_desc<1024>(list, 1024, tid);
  for (int i = tid; i < p.cap && i < 1024; i += 1024) {
    const unsigned long long c = list[i];
    // invalid slots: any permutation of the remaining indices -- hand out total, total+1, ... in order
    p.prop_order[(long long)n * p.cap + i] = n * p.cap + (c ? (int)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull)) : i);
  }
}

// ---------------------------------------------------------------------------------------------
// Box head: softmax + per-class decode + threshold + per-(image,class) sort
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void box_candidates_kernel(const BoxCandParams p) {
  __shared__ unsigned long long list[1024];
  __shared__ unsigned int cnt;
  const int k = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int K = p.K;
  const int np = p.prop_count[n];
  if (tid == 0) cnt = 0;
  __syncthreads();
  unsigned long long comp = 0ull;
  float box[4] = {0.f, 0.f, 0.f, 0.f};
  float score = 0.f;
  if (tid < np && tid < p.cap) {
    const float* pr = p.pred + ((long long)n * p.cap + tid) * p.cs;
    float mx = pr[0];
    for (int c = 1; c <= K; ++c) mx = fmaxf(mx, pr[c]);
    float sum = 0.f;
    for (int c = 0; c <= K; ++c) sum += expf(pr[c] - mx);
    score = rs_fdiv(expf(pr[k] - mx), sum);
    const float* pb = p.prop_boxes + ((long long)n * p.cap + tid) * 4;
    float b[4] = {pb[0], pb[1], pb[2], pb[3]};
    const float* dp = pr + (K + 1) + k * 4;
    float d[4] = {dp[0], dp[1], dp[2], dp[3]};
    apply_deltas(b, d, p.wx, p.wy, p.ww, p.wh, p.scale_clamp, box);
    box[0] = clampf(box[0], 0.f, p.img_w);
    box[1] = clampf(box[1], 0.f, p.img_h);
    box[2] = clampf(box[2], 0.f, p.img_w);
    box[3] = clampf(box[3], 0.f, p.img_h);
    float* db = p.dec_boxes + (((long long)n * p.cap + tid) * K + k) * 4;
    db[0] = box[0]; db[1] = box[1]; db[2] = box[2]; db[3] = box[3];
    p.dec_scores[((long long)n * p.cap + tid) * K + k] = score;
    if (score > p.score_thresh) {
      comp = ((unsigned long long)fkey(score) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)tid);
      atomicAdd(&cnt, 1u);
    }
  }
  list[tid] = comp;
  __syncthreads();
  bitonic_sort_desc<1024>(list, 1024, tid);
  const int c = (int)cnt;
  const long long sb = ((long long)n * K + k) * 1024;
  if (tid == 0) p.seg_count[n * K + k] = c;
  if (tid < c) {
    const int r = (int)(0xFFFFFFFFu - (uint32_t)(list[tid] & 0xFFFFFFFFull));
    const float* db = p.dec_boxes + (((long long)n * p.cap + r) * K + k) * 4;
    float* o = p.seg_boxes + (sb + tid) * 4;
    o[0] = db[0]; o[1] = db[1]; o[2] = db[2]; o[3] = db[3];
    p.seg_roi[sb + tid] = r;
  }
}

// More than RS_DET_GROUP classes: the softmax statistics of every RoI once (BoxCandParams::roi_stat), in the summation order of
// box_candidates_kernel, so that the scores carry the same bits; the per-class kernel then costs one expf per RoI instead of K + 2.
__global__ __launch_bounds__(256) void box_softmax_stat_kernel(const BoxCandParams p) {
  const int n = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x, K = p.K;
  if (r >= p.prop_count[n] || r >= p.cap) return;
  const float* pr = p.pred + ((long long)n * p.cap + r) * p.cs;
  float mx = pr[0];
  for (int c = 1; c <= K; ++c) mx = fmaxf(mx, pr[c]);
  float sum = 0.f;
  for (int c = 0; c <= K; ++c) sum += expf(pr[c] - mx);
  float* st = p.roi_stat + ((long long)n * p.cap + r) * 2;
  st[0] = mx; st[1] = sum;
}

// box_candidates_kernel on the statistics above.  The candidates are compacted before the sort (the keys are unique, so the order they
// arrive in changes nothing) and the sort runs over the entries that exist: most classes of a trained detector hold none.
__global__ __launch_bounds__(1024) void box_candidates_mc_kernel(const BoxCandParams p) {
  __shared__ unsigned long long list[1024];
  __shared__ unsigned int cnt;
  const int k = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int K = p.K;
  const int np = p.prop_count[n];
  if (tid == 0) cnt = 0;
  list[tid] = 0ull;
  __syncthreads();
  if (tid < np && tid < p.cap) {
    const float* pr = p.pred + ((long long)n * p.cap + tid) * p.cs;
    const float* st = p.roi_stat + ((long long)n * p.cap + tid) * 2;
    const float score = rs_fdiv(expf(pr[k] - st[0]), st[1]);
    const float* pb = p.prop_boxes + ((long long)n * p.cap + tid) * 4;
    float b[4] = {pb[0], pb[1], pb[2], pb[3]};
    const float* dp = pr + (K + 1) + k * 4;
    float d[4] = {dp[0], dp[1], dp[2], dp[3]};
    float box[4];
    apply_deltas(b, d, p.wx, p.wy, p.ww, p.wh, p.scale_clamp, box);
    box[0] = clampf(box[0], 0.f, p.img_w);
    box[1] = clampf(box[1], 0.f, p.img_h);
    box[2] = clampf(box[2], 0.f, p.img_w);
    box[3] = clampf(box[3], 0.f, p.img_h);
    float* db = p.dec_boxes + (((long long)n * p.cap + tid) * K + k) * 4;
    db[0] = box[0]; db[1] = box[1]; db[2] = box[2]; db[3] = box[3];
    p.dec_scores[((long long)n * p.cap + tid) * K + k] = score;
    if (score > p.score_thresh)
      list[atomicAdd(&cnt, 1u)] = ((unsigned long long)fkey(score) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)tid);
  }
  __syncthreads();
  const int c = (int)cnt;
  const long long sb = ((long long)n * K + k) * 1024;
  if (tid == 0) p.seg_count[n * K + k] = c;
  if (c == 0) return;                            // uniform
  bitonic_sort_desc<1024>(list, sort_size(c, 64, 1024), tid);
  if (tid < c) {
    const int r = (int)(0xFFFFFFFFu - (uint32_t)(list[tid] & 0xFFFFFFFFull));
    const float* db = p.dec_boxes + (((long long)n * p.cap + r) * K + k) * 4;   // this workgroup's own stores, ordered by the __syncthreads() above (in front of the count), not by the sort
    float* o = p.seg_boxes + (sb + tid) * 4;
    o[0] = db[0]; o[1] = db[1]; o[2] = db[2]; o[3] = db[3];
    p.seg_roi[sb + tid] = r;
  }
}

// Gather NMS survivors of all classes, order by score (ties: lower roi*K+class first), keep the
// first dets_per_image, then detector_postprocess's box part (scale to tile, clip, drop empty).
// det_finish is that last part, by all 1024 threads: `list` holds an image's keys in final order, `total` of them real.
__device__ __forceinline__ void det_finish(const DetMergeParams& p, int n, const unsigned long long* list, int total) {
  __shared__ unsigned char flag[1024];
  __shared__ int dst[1024];
  const int tid = threadIdx.x, K = p.K;
  const int D = p.dets_per_image;
  const int nd = total < D ? total : D;
  float bn[4] = {0, 0, 0, 0}, bo[4] = {0, 0, 0, 0};
  float sc = 0.f;
  int cls = 0, roi = 0;
  bool ok = false;
  if (tid < nd) {
    const uint32_t flat = 0xFFFFFFFFu - (uint32_t)(list[tid] & 0xFFFFFFFFull);
    roi = (int)(flat / (uint32_t)K);
    cls = (int)(flat - (uint32_t)roi * (uint32_t)K);
    const float* db = p.dec_boxes + (((long long)n * p.cap + roi) * K + cls) * 4;
    bn[0] = db[0]; bn[1] = db[1]; bn[2] = db[2]; bn[3] = db[3];
    sc = fkey_inv((uint32_t)(list[tid] >> 32));
    bo[0] = clampf(bn[0] * p.scale_x, 0.f, p.out_w);
    bo[1] = clampf(bn[1] * p.scale_y, 0.f, p.out_h);
    bo[2] = clampf(bn[2] * p.scale_x, 0.f, p.out_w);
    bo[3] = clampf(bn[3] * p.scale_y, 0.f, p.out_h);
    ok = ((bo[2] - bo[0]) > 0.f) && ((bo[3] - bo[1]) > 0.f);
  }
  flag[tid] = ok ? 1 : 0;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int i = 0; i < nd; ++i) { dst[i] = c; c += flag[i]; }
    p.det_count[n] = c;
  }
  __syncthreads();
  if (ok) {
    const long long s = (long long)n * D + dst[tid];
    float* o1 = p.det_boxes_net + s * 4;
    float* o2 = p.det_boxes + s * 4;
    o1[0] = bn[0]; o1[1] = bn[1]; o1[2] = bn[2]; o1[3] = bn[3];
    o2[0] = bo[0]; o2[1] = bo[1]; o2[2] = bo[2]; o2[3] = bo[3];
    p.det_scores[s] = sc;
    p.det_classes[s] = cls;
    if (p.det_roi) p.det_roi[s] = roi;
  }
}

// NMS survivors of classes [k0, k1) of image n into `list` (zeroed, room for 1024 per class) as sort keys; *cnt counts them
__device__ __forceinline__ void det_gather(const DetMergeParams& p, int n, int k0, int k1, unsigned long long* list, unsigned int* cnt) {
  const int tid = threadIdx.x, K = p.K;
  for (int k = k0; k < k1; ++k) {
    int c = p.seg_count[n * K + k];
    if (c > 1024) c = 1024;                       // a segment has 1024 slots
    const long long sb = ((long long)n * K + k) * 1024;
    for (int i = tid; i < c; i += 1024) {
      if (p.keep[sb + i]) {
        const int r = p.seg_roi[sb + i];
        const float sc = p.dec_scores[((long long)n * p.cap + r) * K + k];
        const unsigned pos = atomicAdd(cnt, 1u);
        list[pos] = ((unsigned long long)fkey(sc) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(r * K + k));
      }
    }
  }
}

__global__ __launch_bounds__(1024) void det_merge_kernel(const DetMergeParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* list = (unsigned long long*)smem;   // 8192
  __shared__ unsigned int cnt;
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) cnt = 0;
  for (int i = tid; i < 8192; i += 1024) list[i] = 0ull;
  __syncthreads();
  det_gather(p, n, 0, p.K, list, &cnt);
  __syncthreads();
  bitonic_sort_desc<1024>(list, sort_size(cnt, 1024, 8192), tid);
  det_finish(p, n, list, (int)cnt);
}

// More than RS_DET_GROUP classes: up to K * 1024 survivors per image do not fit one LDS list.  The keys are unique, so the first D of
// an image are among the first D of every group of RS_DET_GROUP classes: one workgroup per (group, image) sorts its group as
// det_merge_kernel does and hands its first D keys on through global memory; a second LAUNCH (not a hand-off inside one: nothing
// orders one workgroup's stores before another's loads across XCDs short of a kernel boundary) sorts an image's partial winners.
__global__ __launch_bounds__(1024) void det_merge_part_kernel(const DetMergeParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* list = (unsigned long long*)smem;   // 8192
  __shared__ unsigned int cnt;
  const int g = blockIdx.x, G = gridDim.x, n = blockIdx.y, tid = threadIdx.x, K = p.K, D = p.dets_per_image;
  const int k0 = g * RS_DET_GROUP, k1 = k0 + RS_DET_GROUP < K ? k0 + RS_DET_GROUP : K;
  int bound = 0;                                          // candidates of the group: at least its survivors
  for (int k = k0; k < k1; ++k) { const int c = p.seg_count[n * K + k]; bound += c < 0 ? 0 : (c > 1024 ? 1024 : c); }
  if (bound <= 0) {                                       // uniform
    if (tid == 0) p.part_count[n * G + g] = 0;
    return;
  }
  const int room = sort_size((unsigned)bound, 1024, 8192);
  if (tid == 0) cnt = 0;
  for (int i = tid; i < room; i += 1024) list[i] = 0ull;
  __syncthreads();
  det_gather(p, n, k0, k1, list, &cnt);
  __syncthreads();
  bitonic_sort_desc<1024>(list, sort_size(cnt, 1024, 8192), tid);
  const int m = (int)cnt < D ? (int)cnt : D;
  if (tid == 0) p.part_count[n * G + g] = m;
  if (tid < m) p.part_keys[((long long)n * G + g) * D + tid] = list[tid];
}

// room: keys of the LDS list, a power of two >= G * D
__global__ __launch_bounds__(1024) void det_merge_final_kernel(const DetMergeParams p, int G, int room) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* list = (unsigned long long*)smem;
  __shared__ int off[RS_DET_FINAL_KEYS / 1024 + 1];
  const int n = blockIdx.x, tid = threadIdx.x, D = p.dets_per_image;
  if (tid == 0) {
    int c = 0;
    for (int g = 0; g < G; ++g) { off[g] = c; c += p.part_count[n * G + g]; }
    off[G] = c;
  }
  for (int i = tid; i < room; i += 1024) list[i] = 0ull;
  __syncthreads();
  const int total = off[G];
  for (int g = 0; g < G; ++g) {
    const int m = off[g + 1] - off[g];
    if (tid < m) list[off[g] + tid] = p.part_keys[((long long)n * G + g) * D + tid];
  }
  __syncthreads();
  bitonic_sort_desc<1024>(list, sort_size((unsigned)total, 1024, room), tid);
  det_finish(p, n, list, total);
}

// exclusive scan of per-image detection counts -> compact entry list for the mask head
__global__ __launch_bounds__(1024) void det_compact_kernel(const int* det_count, int N, int D, int* slot_list, int* total) {
  __shared__ int off[1025];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int c = 0;
    for (int i = 0; i < N; ++i) { off[i] = c; c += det_count[i]; }
    off[N] = c;
    *total = c;
  }
  __syncthreads();
  for (int n = 0; n < N; ++n) {
    const int c = det_count[n];
    for (int i = tid; i < c; i += 1024) slot_list[off[n] + i] = n * D + i;
  }
}

// ---------------------------------------------------------------------------------------------
// Mask predictor (1x1 conv, predicted class only) + sigmoid.  in: [R][S][S][256] fp16
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_predict_kernel(const MaskPredictParams p) {
  const int total = *p.n_entries;
  const int SS = p.S * p.S;
  const int tid = threadIdx.x;
  const int sub = tid & 15;         // 16 lanes per pixel, 16 channels each
  const long long pix = (long long)blockIdx.x * 16 + (tid >> 4);
  const long long npix = (long long)total * SS;
  if (pix >= npix) return;          // whole 16-lane group exits together
  const int entry = (int)(pix / SS);
  const int slot = p.slot_list[entry];
  const int cls = p.det_classes[slot];
  const float* w = p.w + (long long)cls * 256 + sub * 16;
  float xv[16];
  if (p.f32 == 2) {         // split-operand mode: hi + lo planes
    const half_t* x = p.in + pix * 256 + sub * 16;
    const half8 a = *(const half8*)x, b = *(const half8*)(x + 8), al = *(const half8*)(x + p.in_lo), bl = *(const half8*)(x + p.in_lo + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) { xv[i] = (float)a[i] + (float)al[i]; xv[8 + i] = (float)b[i] + (float)bl[i]; }
  } else if (p.f32) {
    const float* x = (const float*)p.in + pix * 256 + sub * 16;
#pragma unroll
    for (int i = 0; i < 16; ++i) xv[i] = x[i];
  } else {
    const half_t* x = p.in + pix * 256 + sub * 16;
    const half8 a = *(const half8*)x, b = *(const half8*)(x + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) { xv[i] = (float)a[i]; xv[8 + i] = (float)b[i]; }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += xv[i] * w[i];
  s += __shfl_xor(s, 8, 16);
  s += __shfl_xor(s, 4, 16);
  s += __shfl_xor(s, 2, 16);
  s += __shfl_xor(s, 1, 16);
  if (sub == 0) {
    const float logit = s + p.b[cls];
    const float prob = rs_fdiv(1.f, 1.f + expf(-logit));
    p.out[(long long)slot * SS + (pix - (long long)entry * SS)] = prob;
  }
}

// logits accumulated by the fused deconv+predictor GEMM -> + class bias -> sigmoid, in place ([slots][S][S])
__global__ __launch_bounds__(256) void mask_sigmoid_kernel(const MaskPredictParams p) {
  const int total = *p.n_entries;
  const int SS = p.S * p.S;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long long)total * SS) return;
  const int entry = (int)(gid / SS);
  const int slot = p.slot_list[entry];
  float* o = p.out + (long long)slot * SS + (gid - (long long)entry * SS);
  const float logit = *o + p.b[p.det_classes[slot]];
  *o = rs_fdiv(1.f, 1.f + expf(-logit));
}

// ---------------------------------------------------------------------------------------------
// paste_masks_in_image: one thread = 8 horizontally adjacent output pixels = one output byte
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void paste_masks_kernel(const PasteParams p) {
  // one thread = one 32-bit word = 32 horizontally adjacent output pixels (4 output bytes, one dword store)
  const int total = *p.n_entries;
  const int Wb = (p.out_w + 7) >> 3;          // bytes per output row
  const int Ww = (Wb + 3) >> 2;               // words per output row
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long per = (long long)p.out_h * Ww;
  if (gid >= (long long)total * per) return;
  const int entry = (int)(gid / per);
  const int rem = (int)(gid - (long long)entry * per);
  const int y = rem / Ww, xw = rem - y * Ww;
  const int slot = p.slot_list[entry];
  const float* bx = p.det_boxes + (long long)slot * 4;
  const float x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
  const float* m = p.probs + (long long)slot * p.S * p.S;
  const int S = p.S;
  unsigned int word = 0;
  // img_y = (y + 0.5 - y0) / (y1 - y0) * 2 - 1 ; iy = ((img_y + 1) * S - 1) / 2
  const float gy = rs_fdiv((float)y + 0.5f - y0, y1 - y0) * 2.f - 1.f;
  const float iy = ((gy + 1.f) * (float)S - 1.f) * 0.5f;
  const float fy = floorf(iy);
  const int iy0 = (int)fy, iy1 = iy0 + 1;
  const float wy1 = iy - fy, wy0 = 1.f - wy1;
  // conservative column range that can sample inside the SxS map (one mask texel of margin on both sides)
  const float margin = rs_fdiv(fabsf(x1 - x0), (float)S) + 1.f;
  const int xa = xw * 32, xz = xa + 31;
  if (iy1 >= 0 && iy0 < S && (float)xz + 0.5f >= fminf(x0, x1) - margin && (float)xa + 0.5f <= fmaxf(x0, x1) + margin) {
    for (int b = 0; b < 32; ++b) {
      const int x = xa + b;
      if (x >= p.out_w) break;
      const float gx = rs_fdiv((float)x + 0.5f - x0, x1 - x0) * 2.f - 1.f;
      const float ix = ((gx + 1.f) * (float)S - 1.f) * 0.5f;
      const float fx = floorf(ix);
      const int ix0 = (int)fx, ix1 = ix0 + 1;
      if (ix1 < 0 || ix0 >= S) continue;
      const float wx1 = ix - fx, wx0 = 1.f - wx1;
      float v = 0.f;
      if (iy0 >= 0 && ix0 >= 0) v += m[iy0 * S + ix0] * (wx0 * wy0);
      if (iy0 >= 0 && ix1 < S) v += m[iy0 * S + ix1] * (wx1 * wy0);
      if (iy1 < S && ix0 >= 0) v += m[iy1 * S + ix0] * (wx0 * wy1);
      if (iy1 < S && ix1 < S) v += m[iy1 * S + ix1] * (wx1 * wy1);
      if (v >= p.threshold) word |= 1u << b;
    }
  }
  uint8_t* o = p.out + (long long)slot * p.out_h * Wb + (long long)y * Wb + xw * 4;
  if ((Wb & 3) == 0) {
    *(unsigned int*)o = word;
  } else {
    for (int k = 0; k < 4 && xw * 4 + k < Wb; ++k) o[k] = (uint8_t)(word >> (8 * k));
  }
}

// ---------------------------------------------------------------------------------------------
// mask crops for the host: plan (sizes + exclusive scan, one workgroup) and copy (one workgroup per slot)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void mask_crop_plan_kernel(const CropParams p) {
  __shared__ unsigned int part[1024];
  __shared__ unsigned long long base_sh;
  const int tid = threadIdx.x;
  const int E = p.n * p.D;
  if (tid == 0) base_sh = 0ull;
  __syncthreads();
  for (int e0 = 0; e0 < E; e0 += 1024) {
    const int e = e0 + tid;
    unsigned int size = 0;
    int x0b = 0, y0 = 0, wb = 0, rows = 0;
    if (e < E) {
      const int i = e / p.D, d = e - i * p.D;
      if (d < p.det_count[i]) {
        const float* b = p.det_boxes + (long long)e * 4;
        // the pasted mask is zero at every pixel whose centre lies outside the box (grid_sample, zeros padding, >= 0.5 of a
        // probability < 1); one pixel of margin covers the rounding of the sample coordinates
        int xa = (int)floorf(fminf(b[0], b[2])) - 1, xz = (int)ceilf(fmaxf(b[0], b[2])) + 1;
        int ya = (int)floorf(fminf(b[1], b[3])) - 1, yz = (int)ceilf(fmaxf(b[1], b[3])) + 1;
        xa = xa < 0 ? 0 : xa; ya = ya < 0 ? 0 : ya;
        xz = xz > p.w - 1 ? p.w - 1 : xz; yz = yz > p.h - 1 ? p.h - 1 : yz;
        if (xz >= xa && yz >= ya) {
          x0b = xa >> 3; wb = (xz >> 3) - x0b + 1; y0 = ya; rows = yz - ya + 1;
          size = (unsigned int)(wb * rows);
        }
      }
    }
    part[tid] = size;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {          // inclusive scan (Hillis-Steele)
      const unsigned int v = tid >= off ? part[tid - off] : 0u;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    const unsigned long long base = base_sh;
    if (e < E) {
      int* r = p.rects + (long long)e * 4;
      r[0] = x0b; r[1] = y0; r[2] = wb; r[3] = rows;
      p.offsets[e] = (unsigned int)(base + part[tid] - size);
    }
    __syncthreads();
    if (tid == 1023) base_sh = base + part[1023];
    __syncthreads();
  }
  if (tid == 0) *p.total = base_sh;
}

__global__ __launch_bounds__(256) void mask_crop_copy_kernel(const CropParams p) {
  const int e = blockIdx.x;
  const int* r = p.rects + (long long)e * 4;
  const int x0b = r[0], y0 = r[1], wb = r[2], rows = r[3];
  const int total = wb * rows;
  if (total == 0) return;
  const uint8_t* src = p.masks + ((long long)e * p.h + y0) * p.Wb + x0b;
  uint8_t* dst = p.data + p.offsets[e];
  for (int idx = threadIdx.x; idx < total; idx += 256) {
    const int rr = idx / wb, c = idx - rr * wb;
    dst[idx] = src[(long long)rr * p.Wb + c];
  }
}

}  // namespace

// ----------------------------------------------------------------------------------------------- launchers
int launch_mask_crops(const CropParams& p, hipStream_t s) {
  RS_CHECK(p.n > 0 && p.D > 0 && p.masks && p.rects && p.offsets && p.total && p.data, RS_ERR_ARG, "mask crops: bad argument");
  hipLaunchKernelGGL(mask_crop_plan_kernel, dim3(1), dim3(1024), 0, s, p);
  hipLaunchKernelGGL(mask_crop_copy_kernel, dim3(p.n * p.D), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_rpn_select(const RpnParams& p, hipStream_t s) {
  const int cap = p.cand_cap ? p.cand_cap : 1024;
  RS_CHECK((cap == 1024 || cap == 2048) && p.topk <= cap && p.A <= RS_MAX_ANCHORS && p.L <= RS_MAX_LEVELS, RS_ERR_UNSUPPORTED,
           "rpn: topk %d / capacity %d / A %d / L %d out of range", p.topk, cap, p.A, p.L);
  RpnParams q = p;
  q.debug = rs_debug().select_debug;
  if (cap == 1024) hipLaunchKernelGGL(rpn_select_kernel<1024>, dim3(p.L, p.N), dim3(1024), 0, s, q);
  else hipLaunchKernelGGL(rpn_select_kernel<2048>, dim3(p.L, p.N), dim3(1024), 0, s, q);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_nms(const NmsParams& p, int segments, hipStream_t s) {
  const int lds = 1024 * 20 + 256 + 1024 * 128;
  const int lds_big = 2048 * 20 + 256;
  static bool done = false;
  if (!done) {
    RS_HIP(hipFuncSetAttribute((const void*)nms_kernel<1024, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    RS_HIP(hipFuncSetAttribute((const void*)nms_kernel<2048, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_big));
    done = true;
  }
  RS_CHECK(p.cap > 0 && p.cap <= 2048 && (p.cap <= 1024 || p.scratch), RS_ERR_ARG, "nms: capacity %d (more than 1024 boxes need NmsParams::scratch)", p.cap);
  RS_CHECK(!p.rule || (p.unit && p.group >= 1 && segments % p.group == 0), RS_ERR_ARG, "nms: %d segments in groups of %d", segments, p.group);
  RS_CHECK(!p.rule || p.cap > 1000, RS_ERR_ARG, "nms: the batched_nms size rule needs a capacity above 1000 boxes per segment, got %d", p.cap);
  NmsParams q = p;
  q.debug = rs_debug().nms_debug;
  // few segments (images x levels / classes) and a quadratic mask build: with one workgroup per segment most of the chip idles, so the rows of a
  // segment are shared by `parts` workgroups (mask in global memory) and the (serial, cheap) scan runs as a second launch.  Same tests, same
  // greedy scan: identical keep flags.
  int parts = segments >= 256 ? 1 : (256 + segments - 1) / segments;
  if (parts > 16) parts = 16;
  if (p.cap <= 1024) {
    if (!p.scratch || segments > 32 || parts == 1) hipLaunchKernelGGL((nms_kernel<1024, false>), dim3(segments), dim3(1024), lds, s, q);
    else {
      if (parts > 8) parts = 8;
      q.mode = 1;
      hipLaunchKernelGGL((nms_kernel<1024, true>), dim3(segments, parts), dim3(1024), 1024 * 20 + 256, s, q);
      q.mode = 2;
      hipLaunchKernelGGL((nms_kernel<1024, true>), dim3(segments), dim3(1024), 1024 * 20 + 256, s, q);
    }
  } else if (parts == 1) {
    q.mode = 0;
    hipLaunchKernelGGL((nms_kernel<2048, true>), dim3(segments), dim3(1024), lds_big, s, q);
  } else {
    q.mode = 1;
    hipLaunchKernelGGL((nms_kernel<2048, true>), dim3(segments, parts), dim3(1024), lds_big, s, q);
    q.mode = 2;
    hipLaunchKernelGGL((nms_kernel<2048, true>), dim3(segments), dim3(1024), lds_big, s, q);
  }
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_rpn_merge(const RpnMergeParams& p, int N, hipStream_t s) {
  const int cap = p.cand_cap ? p.cand_cap : 1024;
  RS_CHECK(p.L <= 8 && (cap == 1024 || cap == 2048), RS_ERR_UNSUPPORTED, "rpn merge: %d levels / capacity %d", p.L, cap);
  static bool done = false;
  if (!done) {
    RS_HIP(hipFuncSetAttribute((const void*)rpn_merge_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    RS_HIP(hipFuncSetAttribute((const void*)rpn_merge_kernel<2048>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    done = true;
  }
  if (cap == 1024) hipLaunchKernelGGL(rpn_merge_kernel<1024>, dim3(N), dim3(1024), 65536, s, p);
  else hipLaunchKernelGGL(rpn_merge_kernel<2048>, dim3(N), dim3(1024), 131072, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_box_candidates(const BoxCandParams& p, int N, hipStream_t s) {
  RS_CHECK(p.cap <= 1024, RS_ERR_UNSUPPORTED, "box head: more than 1024 proposals per image");
  if (p.K <= RS_DET_GROUP) hipLaunchKernelGGL(box_candidates_kernel, dim3(p.K, N), dim3(1024), 0, s, p);
  else {
    RS_CHECK(p.roi_stat, RS_ERR_ARG, "box head: %d classes need BoxCandParams::roi_stat", p.K);
    hipLaunchKernelGGL(box_softmax_stat_kernel, dim3(cdiv(p.cap, 256), N), dim3(256), 0, s, p);
    hipLaunchKernelGGL(box_candidates_mc_kernel, dim3(p.K, N), dim3(1024), 0, s, p);
  }
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int det_merge_check(int K, int D) {
  RS_CHECK(K >= 1 && D <= 1024 &&
               (K <= RS_DET_GROUP || (D >= 1 && det_merge_groups(K) <= RS_DET_FINAL_KEYS / 1024 && det_merge_groups(K) * D <= RS_DET_FINAL_KEYS)), RS_ERR_UNSUPPORTED,
           "det merge: NUM_CLASSES %d with DETECTIONS_PER_IMAGE %d -- at most 1024 detections per image, and above %d classes "
           "ceil(NUM_CLASSES / %d) * DETECTIONS_PER_IMAGE <= %d partial winners", K, D, RS_DET_GROUP, RS_DET_GROUP, RS_DET_FINAL_KEYS);
  return RS_OK;
}

int launch_det_merge(const DetMergeParams& p, int N, hipStream_t s) {
  { const int rc = det_merge_check(p.K, p.dets_per_image); if (rc) return rc; }
  static bool done = false;
  if (!done) {
    RS_HIP(hipFuncSetAttribute((const void*)det_merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    RS_HIP(hipFuncSetAttribute((const void*)det_merge_part_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    RS_HIP(hipFuncSetAttribute((const void*)det_merge_final_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RS_DET_FINAL_KEYS * 8));
    done = true;
  }
  if (p.K <= RS_DET_GROUP) hipLaunchKernelGGL(det_merge_kernel, dim3(N), dim3(1024), 65536, s, p);
  else {
    RS_CHECK(p.part_keys && p.part_count, RS_ERR_ARG, "det merge: %d classes need DetMergeParams::part_keys / part_count", p.K);
    const int G = det_merge_groups(p.K);
    int room = 1024;
    while (room < G * p.dets_per_image) room <<= 1;
    hipLaunchKernelGGL(det_merge_part_kernel, dim3(G, N), dim3(1024), 65536, s, p);
    hipLaunchKernelGGL(det_merge_final_kernel, dim3(N), dim3(1024), room * 8, s, p, G, room);
  }
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_det_compact(const int* det_count, int N, int D, int* slot_list, int* total, hipStream_t s) {
  RS_CHECK(N <= 1024, RS_ERR_UNSUPPORTED, "batch > 1024");
  hipLaunchKernelGGL(det_compact_kernel, dim3(1), dim3(1024), 0, s, det_count, N, D, slot_list, total);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_mask_predict(const MaskPredictParams& p, int capacity_entries, hipStream_t s) {
  const long long npix = (long long)capacity_entries * p.S * p.S;
  hipLaunchKernelGGL(mask_predict_kernel, dim3(cdiv(npix, 16)), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_mask_sigmoid(const MaskPredictParams& p, int capacity_entries, hipStream_t s) {
  const long long npix = (long long)capacity_entries * p.S * p.S;
  hipLaunchKernelGGL(mask_sigmoid_kernel, dim3(cdiv(npix, 256)), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

int launch_paste_masks(const PasteParams& p, int capacity_entries, hipStream_t s) {
  const long long total = (long long)capacity_entries * p.out_h * ((((p.out_w + 7) >> 3) + 3) >> 2);
  hipLaunchKernelGGL(paste_masks_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}
