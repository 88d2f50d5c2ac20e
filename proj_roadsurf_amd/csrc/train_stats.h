// Per-element rules of the training diagnostics (detectron2 0.6: RPN.losses' anchor counts, label_and_sample_proposals' sample
// counts, FastRCNNOutputLayers._log_classification_stats, mask_rcnn_loss' accuracy block), counted as integers.
// Shared by label_counts_kernel / box_stats_kernel / mask_stats_kernel (train_kernels.hip) and the host restatements
// rs_host_label_counts / rs_host_box_stats / rs_host_mask_stats (ops.hip); DESIGN.md section 8 ("Training diagnostics") states them.
//
// Every decision on a float is taken on its BIT PATTERN, so that it does not depend on the denormal mode of whoever compiled the
// caller: `x > 0` is true for the smallest positive denormal, false for both zeros, true for +inf, false for a NaN; the argmax orders
// finite values and infinities as IEEE does, with -0.0 == +0.0, and the FIRST index wins a tie (torch.argmax).  A NaN logit has no
// specified rank (such a step ends through its non-finite loss); nothing here reads outside the K + 1 logits whatever they hold.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif

// int32 train_stats[TS_TABLE] of the trainer; the operators add into the sub-ranges
#define TS_TABLE 16
#define TS_RPN 0        // pos, neg
#define TS_ROI 2        // fg, bg
#define TS_BOX 4        // inst, correct, fgn, fg_correct, fg_as_bg
#define TS_MASK 9       // pixels, incorrect, positive, false_pos, false_neg
#define TS_IMAGES 14    // n
#define TS_MAX_CLASSES 8

TS_HD uint32_t ts_bits(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return b;
}

// x > 0.0f: sign clear, not zero, not a NaN -- bit patterns 0x00000001 .. 0x7f800000
TS_HD bool ts_positive(float x) { return ts_bits(x) - 1u < 0x7f800000u; }

// a key whose unsigned order is the IEEE order of finite values and infinities, with both zeros on one key
TS_HD uint32_t ts_order_key(float x) {
  uint32_t b = ts_bits(x);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// index of the first maximum among row[0 .. K] (K + 1 logits; K = background).  The caller guarantees K + 1 <= the row's width cs.
TS_HD int ts_argmax_first(const float* row, int K) {
  int best = 0;
  uint32_t kb = ts_order_key(row[0]);
  for (int c = 1; c <= K; ++c) {
    const uint32_t k = ts_order_key(row[c]);
    if (k > kb) { kb = k; best = c; }
  }
  return best;
}

// the loss kernels' validity rules: a box row counts with a class in [0, K] (-1 = empty slot), a mask entry with a class in [0, cs)
TS_HD bool ts_box_row_counts(int cls, int K) { return cls >= 0 && cls <= K; }
TS_HD bool ts_mask_entry_counts(int cls, int cs) { return cls >= 0 && cls < cs; }

// one box row -> its five flags (inst, correct, fgn, fg_correct, fg_as_bg)
TS_HD void ts_box_row(const float* row, int cls, int K, int f[5]) {
  f[0] = f[1] = f[2] = f[3] = f[4] = 0;
  if (!ts_box_row_counts(cls, K)) return;
  const int pred = ts_argmax_first(row, K);
  const int fg = cls < K;
  f[0] = 1;
  f[1] = pred == cls;
  f[2] = fg;
  f[3] = fg && pred == cls;
  f[4] = fg && pred == K;
}

// one mask pixel -> its five flags (pixels, incorrect, positive, false_pos, false_neg)
TS_HD void ts_mask_pixel(float logit, uint8_t target, int f[5]) {
  const int p = ts_positive(logit), g = target != 0;
  f[0] = 1;
  f[1] = p != g;
  f[2] = g;
  f[3] = p && !g;
  f[4] = !p && g;
}
