// The optimiser step of one element, stated once: torch.optim.SGD (momentum, weight decay, optional Nesterov, dampening 0) behind
// detectron2 0.6's gradient clipping (solver/build.py: `value` and `norm` per parameter tensor; `full_model`, one norm over all of them,
// is what detectron2's DETR / Mask2Former projects add) and get_default_optimizer_params' bias groups.  Shared by sgd_segments_kernel /
// grad_norm_finish_kernel (train_kernels.hip) and the host restatement rs_host_sgd_segments (ops.hip); DESIGN.md section 8
// ("The optimiser step") states it.
//
//   g = grad * inv_scale                 loss scale and data-parallel divisor: clipping sees the UNSCALED, rank-averaged gradient
//   g = clip(g)                          value: clamp(g, -v, +v)      norm / full_model: g * c      none: c = 1
//   g = g + wd_seg * w
//   b = mu * buf + g
//   d = nesterov ? g + mu * b : b
//   w = w - lr_seg * d ;  buf = b
//
// Every product and sum is rounded to fp32 on its own (no contraction, whatever the including unit is compiled with), in the order of
// sgd_momentum_kernel: with c = 1, no Nesterov and the weights' lr / wd this function returns that kernel's bits (g * 1.0f is g).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SGD_HD __host__ __device__ __forceinline__
#else
#define SGD_HD inline
#endif

// rs_solver.clip_type
#define SGD_CLIP_NONE 0
#define SGD_CLIP_VALUE 1
#define SGD_CLIP_NORM 2
#define SGD_CLIP_FULL_MODEL 3
#define SGD_SEG_BIAS 1        // segment flag: the tensor is a bias (BIAS_LR_FACTOR, WEIGHT_DECAY_BIAS)
#define SGD_CHUNK 8192        // floats per chunk of the flat buffer: one workgroup, 256 lanes x 8 loads of 16 bytes
#define SGD_NORM_EPS 1e-6f    // torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6)

// a run of at most SGD_CHUNK values that lies inside ONE segment, or inside one gap between segments (seg = -1: the weights'
// hyper-parameters, no clipping)
struct SgdChunk {
  long long off;
  int count;
  int seg;
  int flags;
  int pad;
};

// the hyper-parameters of one launch; lr_bias = lr * BIAS_LR_FACTOR and wd_bias are formed once on the host
struct SgdHyper {
  float lr, lr_bias, wd, wd_bias, momentum, inv_scale, clip_value;
  int nesterov, clip_type;
};

// clip: SGD_CLIP_VALUE clamps to +-v (c is not read); every other type multiplies by c (1 where nothing is clipped)
SGD_HD void sgd_rule(float* w, float* buf, float grad, float inv_scale, float lr_seg, float wd_seg, float mu, int nesterov, int clip_value_on,
                     float v, float c) {
#pragma clang fp contract(off)
  float g = grad * inv_scale;
  if (clip_value_on) g = g < -v ? -v : (g > v ? v : g);      // torch.clamp_: a NaN stays a NaN
  else g = g * c;
  g = g + wd_seg * *w;
  const float b = mu * *buf + g;
  const float d = nesterov ? g + mu * b : b;
  *w = *w - lr_seg * d;
  *buf = b;
}

// clip_grad_norm_'s coefficient in its fp32 arithmetic: min(1, max_norm / (norm + 1e-6)).  A zero gradient gives max_norm / 1e-6, which
// clamps to 1; the quotient is the caller's (rs_fdiv on the device, `/` on the host: both correctly rounded)
SGD_HD float sgd_clip_denominator(float norm) {
#pragma clang fp contract(off)
  return norm + SGD_NORM_EPS;
}
SGD_HD float sgd_clip_clamp(float quotient) { return quotient < 1.0f ? quotient : 1.0f; }      // a NaN norm: the step is skipped anyway
