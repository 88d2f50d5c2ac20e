// Training-path kernels (train_kernels.hip): parameter blocks and launchers.
#pragma once
#include <vector>
#include "common.h"
#include "mask_targets.h"
#include "sgd_rule.h"

// Optional scratch of a loss kernel: with it the logged loss is summed in a fixed order (one slot per workgroup, the last workgroup adds
// them) instead of one float atomic per wave, so that two runs of a step report the same bits.  Null partial = the atomics.  One
// scratch per stream of launches: the counter is left at 0 by every launch.
struct LossScratch {
  float* partial;           // [2][cap]
  unsigned int* counter;    // [1], zero before the launch
  int cap;                  // workgroups a launch may have
};
struct RpnLossParams {
  const float* head;        // one level's fused RPN head output [N][HW][cs] fp32: [0,A) logits, [A,5A) deltas
  half_t* dhead;            // gradient, same layout, fp16 (times loss_scale)
  const int* labels;        // [N][total_anchors]: 1 positive, 0 negative, -1 not sampled (after subsampling)
  const float* anchors;     // [total_anchors][4]
  const float* matched_gt;  // [N][total_anchors][4] matched gt box per anchor, or null: gathered from gt/matched below
  const float* gt;          // [N][gt_cap][4]
  const int* matched;       // [N][total_anchors] index of the matched gt
  float* loss_out;          // [2]: loss_rpn_cls, loss_rpn_loc (accumulated)
  int A, cs, dcs, HW, n_anchors, level_off, total_anchors, gt_cap;   // dcs: row stride of dhead (>= 5A; 0 = cs)
  float normalizer;         // BATCH_SIZE_PER_IMAGE * N
  float loss_scale;
  int d32;                  // 1: dhead points to fp32 (reference-precision trainer)
  LossScratch scratch;
};
struct BoxLossParams {
  const float* pred;        // [n_rois][cs] fp32: [0,K] logits (K = background), then 4K deltas
  half_t* dpred;            // gradient fp16 (times loss_scale)
  const int* gt_classes;    // [n_rois]: class, K = background, -1 = empty slot (no loss)
  const float* proposals;   // [n_rois][4]
  const float* gt_boxes;    // [n_rois][4] matched gt box (used for foreground rows)
  float* loss_out;          // [2]: loss_cls, loss_box_reg
  int n_rois, K, cs, dcs;   // dcs: row stride of dpred (0 = cs)
  float n_valid;            // number of sampled RoIs (gt_classes >= 0): the mean's denominator; used when n_valid_counts is null
  const int* n_valid_counts;   // optional device array [n_valid_n][2] (sampled foreground, background per image): n_valid = their sum
  int n_valid_n;
  float wx, wy, ww, wh;
  float loss_scale;
  int d32;                  // 1: dpred points to fp32
  LossScratch scratch;
};
struct MaskLossParams {
  const float* logits;      // [n_masks][S*S][cs] fp32, channel = class
  half_t* dlogits;          // gradient fp16 (times loss_scale)
  const uint8_t* targets;   // [n_masks][S*S] 0/1
  const int* gt_classes;    // [n_masks]
  float* loss_out;          // [1]
  const int* n_masks_ptr;   // optional device count (<= n_masks = capacity): the mean runs over it
  int n_masks, S, cs, dcs;  // dcs: row stride of dlogits (0 = cs)
  float loss_scale;
  int d32;                  // 1: dlogits points to fp32
  LossScratch scratch;
};
int launch_rpn_loss(const RpnLossParams& p, int N, hipStream_t s);
int launch_box_loss(const BoxLossParams& p, hipStream_t s);
int launch_mask_loss(const MaskLossParams& p, hipStream_t s);
int launch_sgd_momentum(float* w, float* buf, const float* grad, long long n, float lr, float momentum, float weight_decay,
                        float inv_loss_scale, int first_step, hipStream_t s, const int* skip = nullptr);
int launch_grad_nonfinite(const float* grad, long long n, int* flag, hipStream_t s);   // flag = 1 if any inf / nan
// The segmented optimiser step (sgd_rule.h): device tables of one flat buffer.  sgd_plan_cut validates a segment table (ascending, no
// overlap, offsets multiples of 4, counts >= 1, inside [0, n), flags 0 / SGD_SEG_BIAS) and cuts [0, n) into chunks, gaps included;
// sgd_plan_pack lays chunks + the {first chunk, chunk count} pair of every segment out as they are uploaded to the front of ONE device
// allocation of sgd_plan_bytes, which sgd_plan_place divides (every part 256-byte aligned).
struct SgdPlan {
  const SgdChunk* chunks;   // [n_chunks]
  const int* seg_chunks;    // [n_seg][2]
  double* partial;          // [n_chunks] grad_norm_partial_kernel's output
  double* seg_sum;          // [n_seg] float64 sum of squares (or the maximum) of every segment
  float* norms;             // [n_seg]
  float* coef;              // [n_seg]
  int n_chunks, n_seg;
};
int sgd_plan_cut(const char* who, const int64_t* seg_off, const int64_t* seg_count, const int32_t* seg_flags, int n_seg, long long n, std::vector<SgdChunk>* chunks,
                 std::vector<int>* seg_chunks);
size_t sgd_plan_table_bytes(int n_chunks, int n_seg);
size_t sgd_plan_bytes(int n_chunks, int n_seg);
void sgd_plan_pack(const std::vector<SgdChunk>& chunks, const std::vector<int>& seg_chunks, std::vector<uint8_t>* host);
SgdPlan sgd_plan_place(void* base, int n_chunks, int n_seg);
// rs_solver (include/rs_engine.h) -> checked, then the hyper-parameters of one launch (ops.hip).  `who` names the entry in the error text.
struct rs_solver;
int sgd_solver_check(const char* who, const rs_solver* sv);
int sgd_solver_hyper(const char* who, const rs_solver& sv, float lr, float momentum, float weight_decay, float inv_scale, SgdHyper* h, int* norm_inf);
int launch_grad_norms(const SgdPlan& p, const float* grad, const SgdHyper& h, int norm_inf, int* flag, hipStream_t s);
int launch_sgd_segments(const SgdPlan& p, float* w, float* buf, const float* grad, const SgdHyper& h, const int* skip, hipStream_t s);
// one layer of the fold (master fp32 -> fp16 GEMM operands); Cout == 0 marks a bias copy (w32 -> fwd32, Cin floats, KH times)
struct FoldDesc {
  const float* w32;
  const float* scale;
  half_t* fwd;
  half_t* bwd;
  float* fwd32;
  int Cout, Cin, KH, KW, Kpad, kc, KpadT;
  unsigned block_start;     // first block of this entry in the table launch
  int f32;                  // 1: fwd / bwd point to fp32 operands (reference-precision trainer: no rounding, same layouts)
};
unsigned fold_desc_blocks(const FoldDesc& d);
int launch_fold_table(const FoldDesc* table_dev, int n_desc, unsigned total_blocks, hipStream_t s);
int launch_fold_weights(const float* w32, const float* scale, half_t* fwd, half_t* bwd, int Cout, int Cin, int KH, int KW, int Kpad,
                        int kc, int KpadT, hipStream_t s);
#define RS_BIAS_GRAD_SLICES 1024  // scratch: RS_BIAS_GRAD_SLICES * cout floats
int launch_bias_grad(const half_t* dy, long long rows, int C, int cout, float* grad, int accumulate, hipStream_t s, const int* m_count,
                     int m_mul, float* scratch, int f32 = 0);
int launch_subsample2_bwd(const half_t* d_coarse, half_t* d_fine, int N, int Hf, int Wf, int Hc, int Wc, int C, hipStream_t s, int f32 = 0);

// ---- backward of the stem (stem_bwd.hip; MODEL.BACKBONE.FREEZE_AT 0)
// max_pool2d(3, 2, 1) backward fused with the ReLU mask of its input: dx = (x > 0) * sum of dq over the windows whose argmax the pixel is
struct PoolBwdParams {
  const void* x;            // [N][Hc + 2 x_halo][Wc + 2 x_halo][C] the pool's input, post-ReLU (fp16, or fp32 with f32)
  const void* dq;           // [N][Hq + 2 q_halo][Wq + 2 q_halo][C] gradient of the pooled map
  void* dx;                 // x's geometry: every interior element written, the halo not touched
  int N, Hc, Wc, Hq, Wq, C, x_halo, q_halo;
  int f32;
};
int launch_maxpool3x3s2_bwd(const PoolBwdParams& p, hipStream_t s);
// weight gradient of the 7x7 stride-2 pad-3 stem convolution in its forward GEMM layout [64][RS_STEM_KPAD]: column (kh * 8 + kw) * 4 + ci
#define RS_STEM_KPAD 256
#define RS_STEM_WGRAD_MAX_SPLITS 512
struct StemWgradParams {
  const void* dy;           // [N][Hc + 2 dy_halo][Wc + 2 dy_halo][64] gradient of the convolution output (fp16, or fp32 with f32)
  const void* x0;           // [N][2 Hc + 2 x_halo][2 Wc + 2 x_halo][4] the network input, x_halo >= 3
  const float* scale;       // [64] FrozenBN scale, or null
  float* partial;           // [splits][64][RS_STEM_KPAD] scratch
  float* grad;              // [64][RS_STEM_KPAD]; the columns of the eighth tap and of the channels >= cin are written as zeros
  int N, Hc, Wc, dy_halo, x_halo, cin, splits;
  int f32;
};
int stem_wgrad_splits(long long pixels);
int launch_stem_wgrad(const StemWgradParams& p, hipStream_t s);

// ---- label assignment (Matcher + subsample_labels) ----
struct MatchParams {
  const float* boxes;       // [n_boxes][4] shared by all images (anchors), or [N][n_boxes][4] when per_image_boxes
  const float* gt;          // [N][gt_cap][4]
  const int* gt_count;      // [N]
  int* matched;             // [N][n_boxes] index of the best gt (0 when the image has none)
  int* labels;              // [N][n_boxes] label of the IoU band: lbl_lo (< t_lo), lbl_mid ([t_lo, t_hi)), lbl_hi (>= t_hi)
  float* best_iou;          // [N][n_boxes] (optional)
  unsigned int* gt_best;    // [N][gt_cap] scratch: bit pattern of every gt's highest IoU (zeroed by the launcher); null = no
                            // low-quality matches
  const int* box_count;     // optional [N]: boxes beyond it get label -1 (per-image proposal lists)
  int n_boxes, gt_cap, per_image_boxes;
  float t_lo, t_hi;
  int lbl_lo, lbl_mid, lbl_hi;
};
struct SubsampleParams {
  int* labels;              // [N][n] in: class / band label; out (rpn_mode): 1 sampled positive, 0 sampled negative, -1 rest
  int* sampled;             // [N][num_samples] (roi mode): sampled indices, positives first, each group ascending; -1 padded
  int* sampled_count;       // [N][2]: number of sampled positives, negatives
  int n, num_samples, bg_label, rpn_mode;
  float positive_fraction;
  unsigned int seed;        // changes every iteration
};
int launch_match(const MatchParams& p, int N, hipStream_t s);
int launch_subsample(const SubsampleParams& p, int N, hipStream_t s);

// ---- RoI-head proposal sampling glue (label_and_sample_proposals)
struct RoiSampleParams {
  const float* prop_boxes;  // [N][prop_cap][4] RPN proposals
  const int* prop_count;    // [N]
  const float* gt_boxes;    // [N][gt_cap][4]
  const int* gt_classes;    // [N][gt_cap]
  const int* gt_count;      // [N]
  float* cand_boxes;        // [N][cand_cap][4]: proposals then the image's gt boxes (PROPOSAL_APPEND_GT, R:193)
  int* cand_count;          // [N]
  int* matched;             // [N][cand_cap] (from the Matcher)
  int* labels;              // [N][cand_cap] in: Matcher label (1 / 0 / -1) -> out: class, K = background, -1 = no candidate
  const int* sampled;       // [N][num_samples] candidate indices (subsample), -1 padded
  const int* sampled_count; // [N][2]
  float* out_boxes;         // [N][out_cap][4] sampled boxes (the box head's proposal buffer)
  int* out_count;           // [N]
  int* out_classes;         // [N][out_cap] class, K = background, -1 = empty slot
  float* out_gt_boxes;      // [N][out_cap][4] matched gt box (foreground rows)
  int* out_gt_index;        // [N][out_cap] matched gt index
  int prop_cap, gt_cap, cand_cap, num_samples, out_cap, K;
};
int launch_roi_candidates(const RoiSampleParams& p, int N, hipStream_t s);
int launch_roi_classes(const RoiSampleParams& p, int N, hipStream_t s);
int launch_roi_gather(const RoiSampleParams& p, int N, hipStream_t s);

// foreground RoIs of the sampled set -> compact mask-head entry list
struct MaskEntriesParams {
  const int* sampled_count; // [N][2]
  const int* roi_classes;   // [N][slots_per_image]
  int* slots;               // [cap] out: slot = n * slots_per_image + j, image-major, j ascending
  int* classes;             // [cap] out
  int* total;               // [1] out
  int N, slots_per_image, per_image_cap, cap;
};
int launch_mask_entries(const MaskEntriesParams& p, hipStream_t s);

// ground-truth masks of the mask-head entries on the device (mask_targets.h): one workgroup per entry.
// Trainer form (slots != null): entry e < *total is slot slots[e] of the sampled RoI list -- box boxes[slot], instance
// image_first[slot / slots_per_image] + gt_index[slot].  Explicit form (slots == null): entry e is instance gt_index[e] of n_inst
// inside boxes[e].  An instance index outside its range gives an all-zero mask and reads no polygon.
struct MaskTargetsParams {
  const float* boxes;       // [..][4] x1, y1, x2, y2
  const int* gt_index;
  const int* slots;         // [n_entries] or null
  const int* total;         // [1] device entry count (trainer form)
  const int* image_first;   // [images + 1] first instance of every image (trainer form)
  const double* polys;      // polygon pool: polygon q = poly_len[q] doubles (x0, y0, x1, y1, ...) at polys + poly_off[q]
  const int* poly_off;
  const int* poly_len;
  const int* inst_first;    // [instances + 1] first polygon of every instance
  uint8_t* out;             // [n_entries][S*S] 0/1, row-major, 4-byte aligned
  int n_entries, n_inst, slots_per_image, S;
};
int launch_mask_targets(const MaskTargetsParams& p, hipStream_t s);

// ---- training diagnostics (train_stats.h): integer counts ADDED into the caller's table, at most one atomicAdd per workgroup and
// counter, so that two runs give the same table.  Nothing here writes a gradient or a loss.
struct LabelCountsParams {
  const int* labels;        // [count]: 1 positive, 0 negative, anything else not sampled
  int count;
  int* out;                 // [2] += pos, neg
  int* images_out;          // optional [1] += images (the trainer's table carries the step's n)
  int images;
};
struct BoxStatsParams {
  const float* pred;        // [n_rois][cs] fp32: [0,K] logits (K = background); the deltas behind them are not read
  const int* gt_classes;    // [n_rois]: class, K = background, anything outside [0, K] does not count
  const int* sampled_counts;   // optional [n_images][2] (sampled foreground, background per image)
  int* out;                 // [7] += fg, bg (from sampled_counts), inst, correct, fgn, fg_correct, fg_as_bg
  int n_rois, K, cs, n_images;
};
struct MaskStatsParams {
  const float* logits;      // [n_masks][S*S][cs] fp32, channel = class
  const uint8_t* targets;   // [n_masks][S*S]
  const int* gt_classes;    // [n_masks]: an entry with a class outside [0, cs) does not count
  const int* n_masks_ptr;   // optional device count, clamped to n_masks (= capacity)
  int* out;                 // [5] += pixels, incorrect, positive, false_pos, false_neg
  int n_masks, S, cs;
};
int launch_label_counts(const LabelCountsParams& p, hipStream_t s);
int launch_box_stats(const BoxStatsParams& p, hipStream_t s);
int launch_mask_stats(const MaskStatsParams& p, hipStream_t s);
