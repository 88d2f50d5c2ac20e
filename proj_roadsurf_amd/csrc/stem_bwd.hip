// Backward of the stem (MODEL.BACKBONE.FREEZE_AT 0): the two kernels the trainer needs below res2.
//  * maxpool3x3s2_bwd_kernel: gradient of max_pool2d(3, 2, 1) fused with the stem's ReLU mask, owner-computes, no atomics.
//  * stem_wgrad_kernel + stem_wgrad_reduce_kernel: weight gradient of the 7x7 stride-2 convolution on 4 padded input channels, written
//    in the stem's forward GEMM layout [64][(kh, kw padded to 8, ci padded to 4)] = [64][256].
// Launchers and parameter blocks: train.h.  Operators: rs_op_maxpool3x3s2_bwd, rs_op_stem_wgrad(_f32) (ops.hip).
#include "train.h"

namespace {

// ---------------------------------------------------------------------------------------------
// d_stem_conv = relu'(stem_conv) * max_pool2d_backward(d_pool), in stem_conv's geometry.
// One thread owns a 2 x 2 block of input pixels (rows 2a, 2a+1; columns 2b, 2b+1) times 16 bytes of channels.  The only windows that
// contain one of them are (a + wy, b + wx), wy, wx in {0, 1}; together they cover the 5 x 5 input patch at (2a - 1, 2b - 1), which the
// thread reads once into registers (neighbouring threads share 3 of its 5 rows and columns through L1 / L2).  Per channel it recomputes
// the argmax of the four windows by ATen's rule (max_pool2d_with_indices: scan in (row, column) order, a later element replaces the
// current one only if it is strictly greater or NaN, padding positions never take part) and gives every pixel the sum, in fp32 and in
// ascending (oy, ox) order -- ATen's CPU scatter order -- of the d_pool of the windows whose argmax it is: pixel (even, even) lies in one
// window, (even, odd) and (odd, even) in two, (odd, odd) in four.  The halo of neither tensor is read or written.
// ---------------------------------------------------------------------------------------------
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const PoolBwdParams p) {
  typedef T TV __attribute__((ext_vector_type(V)));
  const int cv = p.C / V;
  const int A = (p.Hc + 1) >> 1, B = (p.Wc + 1) >> 1;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)p.N * A * B * cv;
  if (gid >= total) return;
  const int c0 = (int)(gid % cv) * V;
  long long t = gid / cv;
  const int b = (int)(t % B); t /= B;
  const int a = (int)(t % A);
  const int n = (int)(t / A);
  const int xHp = p.Hc + 2 * p.x_halo, xWp = p.Wc + 2 * p.x_halo;
  const int qHp = p.Hq + 2 * p.q_halo, qWp = p.Wq + 2 * p.q_halo;
  const T* x = (const T*)p.x;
  const T* dq = (const T*)p.dq;
  T* dx = (T*)p.dx;
  bool rv[5], cl[5];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    rv[r] = 2 * a - 1 + r >= 0 && 2 * a - 1 + r < p.Hc;
    cl[r] = 2 * b - 1 + r >= 0 && 2 * b - 1 + r < p.Wc;
  }
  TV pt[5][5];
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      TV v;
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = (T)0.f;
      if (rv[r] && cl[c]) v = *(const TV*)(x + (((long long)n * xHp + 2 * a - 1 + r + p.x_halo) * xWp + 2 * b - 1 + c + p.x_halo) * p.C + c0);
      pt[r][c] = v;
    }
  int am[2][2][V];      // patch position 5 r + c of the window's argmax, -1 = the window does not exist
  TV g[2][2];
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {
      const bool wok = a + wy < p.Hq && b + wx < p.Wq;
      TV gv;
#pragma unroll
      for (int i = 0; i < V; ++i) gv[i] = (T)0.f;
      if (wok) gv = *(const TV*)(dq + (((long long)n * qHp + a + wy + p.q_halo) * qWp + b + wx + p.q_halo) * p.C + c0);
      g[wy][wx] = gv;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float best = 0.f;
        int idx = -1;
#pragma unroll
        for (int r = 2 * wy; r < 2 * wy + 3; ++r)
#pragma unroll
          for (int c = 2 * wx; c < 2 * wx + 3; ++c) {
            const float f = (float)pt[r][c][i];
            const bool take = rv[r] && cl[c] && (idx < 0 || f > best || f != f);
            best = take ? f : best;
            idx = take ? 5 * r + c : idx;
          }
        am[wy][wx][i] = wok ? idx : -1;
      }
    }
#pragma unroll
  for (int py = 0; py < 2; ++py)
#pragma unroll
    for (int px = 0; px < 2; ++px) {
      if (2 * a + py >= p.Hc || 2 * b + px >= p.Wc) continue;
      const int pos = 5 * (1 + py) + 1 + px;
      TV o;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int wy = 0; wy <= py; ++wy)
#pragma unroll
          for (int wx = 0; wx <= px; ++wx) acc += am[wy][wx][i] == pos ? (float)g[wy][wx][i] : 0.f;
        o[i] = (float)pt[1 + py][1 + px][i] > 0.f ? (T)acc : (T)0.f;
      }
      *(TV*)(dx + (((long long)n * xHp + 2 * a + py + p.x_halo) * xWp + 2 * b + px + p.x_halo) * p.C + c0) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// grad[co][(kh, kw, ci)] = scale[co] * sum over (n, y, x) of dy[n][y][x][co] * x0[n][2y + kh - 3][2x + kw - 3][ci]
// The structure of conv_wgrad_f32_kernel (conv_wgrad.hip): exact fp32 products on v_mfma_f32_16x16x4_f32, both operands read straight
// from global memory, four pixels per step.  Lane (c = lane & 15, q = lane >> 4) loads 16 bytes (8 of fp16 operands) of pixel m + q from
// each side: channels 4c .. 4c+3 of dY, and ONE input pixel of x0 (its 4 padded channels) -- tap (kh = 2 wave + (c >> 3), kw = c & 7).
// So a wave holds the 64 x 64 tile of columns [64 wave, 64 wave + 64) = tap rows 2 wave, 2 wave + 1, and the four waves of a workgroup
// the whole [64][256] matrix; the padding taps (kw = 7, kh = 7) and channels (ci >= cin) read a valid neighbour and are masked to zero.
// The pixel range is split over gridDim.x; every split writes its own fp32 partial matrix, stem_wgrad_reduce_kernel sums them in a
// fixed order, applies the scale and writes exact zeros into the padding columns.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 ld4(const half_t* p) {
  const half4 h = *(const half4*)p;
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

template <typename T>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const StemWgradParams p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = p.N * p.Hc * p.Wc;
  const int steps = (M + 3) >> 2;
  const int per = (steps + (int)gridDim.x - 1) / (int)gridDim.x;
  const int s0 = blockIdx.x * per;
  const int s1 = s0 + per < steps ? s0 + per : steps;
  const int lq = lane >> 4, lc = lane & 15;
  const int kh = 2 * wave + (lc >> 3), kw = lc & 7;
  const bool tap_ok = kh < 7 && kw < 7;
  const int khc = kh < 7 ? kh : 6, kwc = kw < 7 ? kw : 6;
  const int dy_Hp = p.Hc + 2 * p.dy_halo, dy_Wp = p.Wc + 2 * p.dy_halo;
  const int in_Hp = 2 * p.Hc + 2 * p.x_halo, in_Wp = 2 * p.Wc + 2 * p.x_halo, in_off = p.x_halo - 3;
  const T* dy = (const T*)p.dy;
  const T* x = (const T*)p.x0;
  f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // straight-line loop body as in conv_wgrad_f32_kernel: loads from clamped (always valid) addresses, masks applied by selects
  int m = s0 * 4 + lq;
  int xx = m % p.Wc, y, n;
  { const int row = m / p.Wc; y = row % p.Hc; n = row / p.Hc; }
  const int q4 = 4 / p.Wc, r4 = 4 - q4 * p.Wc;          // a step advances the pixel by 4 = q4 rows + r4 columns (launcher: q4 < Hc)
  const int last_row = (M - 1) / p.Wc, last_x = (M - 1) - last_row * p.Wc, last_n = last_row / p.Hc, last_y = last_row - last_n * p.Hc;
  auto load = [&](f32x4& a, f32x4& b, bool& ok) {
    ok = m < M;
    const int yc = ok ? y : last_y, nc = ok ? n : last_n, xc = ok ? xx : last_x;
    a = ld4(dy + ((long long)(nc * dy_Hp + yc + p.dy_halo) * dy_Wp + xc + p.dy_halo) * 64 + 4 * lc);
    b = ld4(x + ((long long)(nc * in_Hp + 2 * yc + khc + in_off) * in_Wp + 2 * xc + kwc + in_off) * 4);
    m += 4;
    xx += r4;
    const bool wx = xx >= p.Wc;
    xx = wx ? xx - p.Wc : xx;
    y += q4 + (wx ? 1 : 0);
    const bool wy = y >= p.Hc;
    y = wy ? y - p.Hc : y;
    n += wy ? 1 : 0;
  };
  auto mfma16 = [&](f32x4 a, f32x4 b, bool ok) {
    const bool okb = ok && tap_ok;
#pragma unroll
    for (int t = 0; t < 4; ++t) { a[t] = ok ? a[t] : 0.f; b[t] = okb && t < p.cin ? b[t] : 0.f; }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[j], acc[t][j], 0, 0, 0);
  };
  f32x4 a0, b0, a1, b1, a2, b2, a3, b3;
  bool k0 = false, k1 = false, k2 = false, k3 = false;
  int s = s0;
  if (s + 1 < s1) {
    load(a0, b0, k0);
    load(a1, b1, k1);
    for (; s + 5 < s1; s += 4) {             // steps s, s+1 are loaded; s+2 .. s+5 exist
      load(a2, b2, k2);
      load(a3, b3, k3);
      __builtin_amdgcn_sched_barrier(0);
      mfma16(a0, b0, k0);
      mfma16(a1, b1, k1);
      __builtin_amdgcn_sched_barrier(0);
      load(a0, b0, k0);
      load(a1, b1, k1);
      __builtin_amdgcn_sched_barrier(0);
      mfma16(a2, b2, k2);
      mfma16(a3, b3, k3);
      __builtin_amdgcn_sched_barrier(0);
    }
    mfma16(a0, b0, k0);
    mfma16(a1, b1, k1);
    s += 2;
  }
  for (; s < s1; ++s) {                      // at most four steps left
    load(a0, b0, k0);
    mfma16(a0, b0, k0);
  }
  float* out = p.partial + (long long)blockIdx.x * 64 * RS_STEM_KPAD;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = 4 * (4 * lq + e) + t;
      *(f32x4*)(out + (long long)co * RS_STEM_KPAD + wave * 64 + 4 * lc) = f32x4{acc[t][0][e], acc[t][1][e], acc[t][2][e], acc[t][3][e]};
    }
}

// grad[co][k] = scale[co] * sum_z partial[z][co][k] in the order of wgrad_reduce_kernel (conv_wgrad.hip): a block owns 64 consecutive
// elements, wave g sums the planes z = g, g + 4, ..., and the four sums are added as ((g0 + g1) + g2) + g3.  Padding columns: +0.
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* partial, int splits, const float* scale, float* grad, int cin) {
  __shared__ float part[4][64];
  const int g = threadIdx.x >> 6, e = threadIdx.x & 63;
  const int i = blockIdx.x * 64 + e;         // < 64 * RS_STEM_KPAD: the grid is exact
  float s = 0.f;
  for (int z = g; z < splits; z += 4) s += partial[(long long)z * 64 * RS_STEM_KPAD + i];
  part[g][e] = s;
  __syncthreads();
  if (g != 0) return;
  s = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  if (scale) s *= scale[i / RS_STEM_KPAD];
  const int col = i % RS_STEM_KPAD;
  const bool real = (col >> 5) < 7 && ((col >> 2) & 7) < 7 && (col & 3) < cin;
  grad[i] = real ? s : 0.f;
}

}  // namespace

int launch_maxpool3x3s2_bwd(const PoolBwdParams& p, hipStream_t s) {
  RS_CHECK(p.x && p.dq && p.dx, RS_ERR_ARG, "maxpool3x3s2_bwd: null operand");
  RS_CHECK(p.N >= 1 && p.Hc >= 1 && p.Wc >= 1 && p.x_halo >= 0 && p.q_halo >= 0 && p.Hq == (p.Hc - 1) / 2 + 1 && p.Wq == (p.Wc - 1) / 2 + 1, RS_ERR_ARG,
           "maxpool3x3s2_bwd: geometry (%d x %d x %d input, %d x %d pooled: a 3x3 stride-2 pad-1 pool gives %d x %d)", p.N, p.Hc, p.Wc, p.Hq, p.Wq,
           (p.Hc - 1) / 2 + 1, (p.Wc - 1) / 2 + 1);
  const int V = p.f32 ? 4 : 8;
  RS_CHECK(p.C >= V && p.C % V == 0, RS_ERR_ARG, "maxpool3x3s2_bwd: %d channels (a multiple of %d: 16-byte pieces)", p.C, V);
  const long long total = (long long)p.N * ((p.Hc + 1) / 2) * ((p.Wc + 1) / 2) * (p.C / V);
  RS_CHECK(total < (1ll << 31) * 256, RS_ERR_ARG, "maxpool3x3s2_bwd: too many elements");
  if (p.f32) hipLaunchKernelGGL((maxpool3x3s2_bwd_kernel<float, 4>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, p);
  else hipLaunchKernelGGL((maxpool3x3s2_bwd_kernel<half_t, 8>), dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  return RS_OK;
}

// splits of the pixel range: at least 32 steps (128 pixels) each, two workgroups per CU of a 256-CU chip at the most
int stem_wgrad_splits(long long pixels) {
  long long s = (pixels + 3) / 4 / 32;
  if (s < 1) s = 1;
  return (int)(s < RS_STEM_WGRAD_MAX_SPLITS ? s : RS_STEM_WGRAD_MAX_SPLITS);
}

int launch_stem_wgrad(const StemWgradParams& p, hipStream_t s) {
  RS_CHECK(p.dy && p.x0 && p.partial && p.grad, RS_ERR_ARG, "stem_wgrad: null operand");
  RS_CHECK(p.N >= 1 && p.Hc >= 1 && p.Wc >= 1 && p.dy_halo >= 0 && p.x_halo >= 3 && p.cin >= 1 && p.cin <= 4, RS_ERR_ARG,
           "stem_wgrad: geometry (%d x %d x %d gradient, halos %d / %d (input: at least 3), %d input channels of 4)", p.N, p.Hc, p.Wc, p.dy_halo, p.x_halo, p.cin);
  RS_CHECK((long long)p.N * p.Hc * p.Wc < (1ll << 31) - 8 && 4 / p.Wc < p.Hc, RS_ERR_ARG, "stem_wgrad: %d x %d x %d pixels", p.N, p.Hc, p.Wc);
  RS_CHECK(p.splits >= 1 && p.splits <= RS_STEM_WGRAD_MAX_SPLITS, RS_ERR_ARG, "stem_wgrad: %d splits outside [1, %d]", p.splits, RS_STEM_WGRAD_MAX_SPLITS);
  if (p.f32) hipLaunchKernelGGL(stem_wgrad_kernel<float>, dim3((unsigned)p.splits), dim3(256), 0, s, p);
  else hipLaunchKernelGGL(stem_wgrad_kernel<half_t>, dim3((unsigned)p.splits), dim3(256), 0, s, p);
  RS_HIP(hipGetLastError());
  hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(64 * RS_STEM_KPAD / 64), dim3(256), 0, s, p.partial, p.splits, p.scale, p.grad, p.cin);
  RS_HIP(hipGetLastError());
  return RS_OK;
}
