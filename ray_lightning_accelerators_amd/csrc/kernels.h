// Host-callable launch API of the HIP kernels (plain pointers + hipStream_t).
// The torch bindings (bindings.cpp) are the only caller; keeping this header
// free of torch types lets the .hip files compile with hipcc alone.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>

namespace rla {

struct AdamArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint16_t* p_bf16;        // optional bf16 copy-out of the updated params
  int64_t n;
  float lr, beta1, beta2, eps, weight_decay, grad_scale;
  int adamw, maximize;
  const int64_t* step_ptr;  // device step counter (already incremented) or null
  int64_t host_step;        // used when step_ptr is null
  const float* lr_ptr;      // device learning rate (graph-replay friendly) or null
};

struct SGDArgs {
  float* p;
  const float* g;
  float* buf;
  uint16_t* p_bf16;
  int64_t n;
  float lr, momentum, dampening, weight_decay, grad_scale;
  int nesterov, maximize;
  const int64_t* step_ptr;
  int64_t host_step;
  const float* lr_ptr;
};

// Param groups that interleave in the arena (sgd_groups_kernel / adam_groups_kernel): ONE
// launch walks a device chunk table of 3 x int64 rows {arena element offset, element count,
// group index}, one workgroup per row.  A row lies inside one group, starts on a multiple of
// 4 elements and holds at most kOptGroupChunk of them; elements that no row covers are
// neither read nor written.  Each group's hyper-parameters travel by value; its step counter
// and learning rate are read from step_ptr[group] / lr_ptr[group] when those are given.
constexpr int kOptMaxGroups = 8;
constexpr int kOptGroupChunk = 16384;

struct AdamGroupHyper {
  float lr, beta1, beta2, eps, weight_decay;
  int adamw, maximize;
  int64_t host_step;  // used when step_ptr is null
};

struct SGDGroupHyper {
  float lr, momentum, dampening, weight_decay;
  int nesterov, maximize;
  int64_t host_step;
};

struct AdamGroupsArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  uint16_t* p_bf16;         // optional, arena-shaped
  int64_t n;                // elements of p: no row may reach beyond it
  const int64_t* table;     // device [rows, 3]
  float grad_scale;
  int ngroups;
  const int64_t* step_ptr;  // device [ngroups] (already incremented) or null
  const float* lr_ptr;      // device [ngroups] or null
  AdamGroupHyper h[kOptMaxGroups];
};

struct SGDGroupsArgs {
  float* p;
  const float* g;
  float* buf;               // arena-shaped; may be null when no group has momentum
  uint16_t* p_bf16;
  int64_t n;
  const int64_t* table;
  float grad_scale;
  int ngroups;
  const int64_t* step_ptr;
  const float* lr_ptr;
  SGDGroupHyper h[kOptMaxGroups];
};

void launch_adam(const AdamArgs& a, hipStream_t stream);
void launch_sgd(const SGDArgs& a, hipStream_t stream);
// -1: ngroups outside [1, kOptMaxGroups]; rows <= 0 launches nothing
int launch_adam_groups(const AdamGroupsArgs& a, int64_t rows, hipStream_t stream);
int launch_sgd_groups(const SGDGroupsArgs& a, int64_t rows, hipStream_t stream);
void launch_multi_copy(const int64_t* table, int64_t nchunks, float scale, int accumulate,
                       hipStream_t stream);
void launch_scale(float* x, int64_t n, float s, hipStream_t stream);
void launch_sumsq(const float* x, int64_t n, float* out, hipStream_t stream);
// Fixed-order sum of squares: part[b] = sum of g[i]^2 over block b's contiguous slice
// (b < nblk <= kClipMaxBlocks; an empty slice gives 0).  No atomics and no memset: the
// same input gives the same bits on every call.  g 16-byte aligned.  -1: bad nblk.
int launch_clip_partials(const float* g, int64_t n, float* part, int nblk, hipStream_t stream);

// ---------------------------------------------------------------------------
// Fused BatchNorm(+ReLU)(+residual add) over NHWC bf16 activations viewed as
// [M, C] rows (csrc/bn_act.hip).  C % 8 == 0 and C <= kBnMaxC.
// ---------------------------------------------------------------------------
constexpr int kBnThreads = 256;

// NHWC bf16 max pooling with a one-byte window argmax (csrc/pool.hip)
// bn_ss (or null): x is a BatchNorm's input, pooled as bf16(relu(x * ss[2] + ss[3])) (the stem's
// BatchNorm + ReLU folded into the pool); nbt_inc as launch_bn_apply's
int launch_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* arg, int N, int H, int W, int C, int OH, int OW,
                       int k, int s, int pad, hipStream_t stream, const float* bn_ss = nullptr,
                       int64_t* nbt_inc = nullptr);
int launch_maxpool_bwd(const uint16_t* dy, const uint8_t* arg, uint16_t* dx, int N, int H, int W, int C, int OH,
                       int OW, int k, int s, int pad, hipStream_t stream);
// global average pool backward over NHWC rows: dx[n][p][c] = dy[n][c] / HW
int launch_gap_bwd(const uint16_t* dy, uint16_t* dx, int N, int HW, int C, hipStream_t stream);
// d [N, H, W, C] += g [N, OH, OW, C] at every s-th pixel (NHWC bf16, fp32 add)
int launch_strided_add(uint16_t* d, const uint16_t* g, int N, int H, int W, int C, int OH, int OW, int s,
                       hipStream_t stream);
// a max pool's backward seen from the layer before it (csrc/pool_gather.h)
struct PoolGrad {
  const uint16_t* g;   // gradient of the pooled output [N, OH, OW, C] bf16
  const uint8_t* arg;  // window argmax bytes [N, OH, OW, C]
  int H, W, OH, OW, k, s, pad;
};
constexpr int kBnMaxC = 2048;  // 8 channels per thread x 256 threads per row

struct BnPlan {
  int64_t rows_per_blk;  // rows each block of the partial kernels reduces
  int blocks;
  int group;   // > 1: blocks per group of the in-kernel second reduction level (fp64 rows)
  int groups;  // ceil(blocks / group): rows the finalize reads
};
BnPlan bn_plan(int64_t M, int C);
// second reduction level of the partial kernels (see bn_act.hip BnL2)
struct BnLevel2 {
  double* rows;  // [groups, 2, C] or nullptr (single level)
  int* tickets;  // [groups] zero-initialised, self-resetting
};

// per-block partial sums part[b][0][c], part[b][1][c]:
//   mode 0 (forward):  sum x, sum x^2   (nbt, if given, is incremented by block 0)
//   mode 1 (backward): sum dz, sum dz*x with dz = dy * (y > 0 if relu)
void launch_bn_partial(const uint16_t* x, const uint16_t* y, const uint16_t* dy, int64_t M, int C, int mode,
                       bool relu, const BnPlan& plan, float* part, int64_t* nbt, hipStream_t s,
                       const uint16_t* dy2 = nullptr,   // backward: gradient = dy + dy2
                       const float* ss = nullptr,       // backward ReLU mask from the fwd stats, not y
                       BnLevel2 l2 = BnLevel2{nullptr, nullptr},
                       uint16_t* dout = nullptr,        // backward: also write d = masked dy (+dy2), bf16
                       const PoolGrad* pool = nullptr);  // backward: dy gathered through a max pool (relu, ss)

// forward finalize of `nparts` partial rows: stats[0]=mean [1]=invstd [2]=scale [3]=shift ([4, C]);
// running stats update (momentum < 0: cumulative average over num_batches_tracked)
void launch_bn_finalize(const float* part, int nparts, int C, double count, const float* gamma,
                        const float* beta, float* running_mean, float* running_var, const int64_t* nbt,
                        float momentum, float eps, float* stats, hipStream_t s,
                        int nbt_pending = 0);  // 1: nbt's += 1 is still to come (bn_apply's nbt_inc)
// the same from the fp64 rows of the second reduction level
void launch_bn_finalize64(const double* part, int nparts, int C, double count, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, const int64_t* nbt,
                          float momentum, float eps, float* stats, hipStream_t s);

// backward finalize: coef[0]=dgamma [1]=dbeta [2]=A [3]=B [4]=Cc ([5, C]); dx = A*dz + B*x + Cc
void launch_bn_bwd_finalize(const float* part, int nparts, int C, double count, const float* gamma,
                            const float* mean, const float* invstd, float* coef, hipStream_t s);
void launch_bn_bwd_finalize64(const double* part, int nparts, int C, double count, const float* gamma,
                              const float* mean, const float* invstd, float* coef, hipStream_t s);

// y = act(x*scale + shift (+ res))
void launch_bn_apply(const uint16_t* x, const uint16_t* res, const float* scale, const float* shift, int64_t M,
                     int C, bool relu, uint16_t* y, hipStream_t s,
                     int64_t* nbt_inc = nullptr);  // block 0 adds 1 (statistics came from a conv epilogue)

// dz = dy * (y > 0 if relu); dx = A*dz + B*x + Cc; dres = dz (if dres)
void launch_bn_bwd_apply(const uint16_t* x, const uint16_t* y, const uint16_t* dy, const float* coef, int64_t M,
                         int C, bool relu, uint16_t* dx, uint16_t* dres, hipStream_t s,
                         const uint16_t* dy2 = nullptr,  // gradient = dy + dy2
                         const float* ss = nullptr,      // ReLU mask from the fwd stats [4, C], not y
                         const PoolGrad* pool = nullptr);  // dy gathered through a max pool (relu, ss)

// 1x1 / stride-1 conv forward y[M][N] = x[M][K] . w[N][K]^T with the next BatchNorm's
// partial sums of bf16(y) in the epilogue: part [gx, 2, N] fp32, bn_finalize's layout
// (csrc/conv1x1.hip)
struct Conv1x1Plan {
  int tnw;            // 32-channel blocks per wave (1 or 2)
  int gy;             // channel columns of 64 tnw
  int gx;             // pixel ranges = partial rows (multiple of 8)
  int tiles_per_blk;  // 128-pixel tiles per range
};
bool conv1x1_stats_ok(int64_t M, int K, int N);
// pre_ss ([4, K] BatchNorm stats, K <= 512): x is a deferred BatchNorm + ReLU's input,
// each x fragment becomes bf16(relu(x * scale + shift)) in the kernel (nbt_inc += 1)
bool conv1x1_pre_ok(int64_t M, int K, int N);
// bwd: launch_conv1x1_bn_bwd's plan (32-channel wave columns whatever N)
Conv1x1Plan conv1x1_stats_plan(int64_t M, int N, bool bwd = false);
// the weight path launch_conv1x1_stats takes: 0 resident beside a 6-stage x ring (<= 16 KB
// weight block), 1 resident beside 4 stages (<= 32 KB), 2 streamed with x
int conv1x1_variant(int K, const Conv1x1Plan& p);
void launch_conv1x1_stats(const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t M, int K, int N,
                          const Conv1x1Plan& p, float* part, hipStream_t s, const float* pre_ss = nullptr,
                          int64_t* nbt_inc = nullptr);
// input gradient of a 1x1 conv (dy1 [M][K] . W, wt = W^T [N][K]) fused with the previous
// BatchNorm's backward partial: d = (da + dy2) * (yb > 0) written to d, part [rows, 2, N]
// = sums of d and d * xb.  part == nullptr: only *rows is set (the partial row count).
bool conv1x1_bn_bwd_ok(int64_t M, int K, int N);
void launch_conv1x1_bn_bwd(const uint16_t* dy1, const uint16_t* wt, uint16_t* d, int64_t M, int K, int N,
                           const uint16_t* dy2, const uint16_t* yb, const uint16_t* xb, float* part, int* rows,
                           hipStream_t s);

// ---------------------------------------------------------------------------
// Fused MNIST-MLP training step (784 -> L1 -> L2 -> 10, ReLU, log_softmax+NLL).
// ---------------------------------------------------------------------------
// The u8 -> bf16 conversion of every MLP kernel: bf16(fmaf((float)u8, x_scale, x_shift)).
// Defaults (ToTensor alone): kMLPXScale, 0 -- bitwise the former u8 * (1.0f / 255.0f) for
// every byte.  A single-channel Normalize(mean, std) folds in as x_scale = 1 / (255 std),
// x_shift = -mean / std.  Padded rows stay zero, not x_shift.
constexpr float kMLPXScale = (float)(1.0 / 255.0);
// what every launch accepts: a finite positive scale, a finite shift
inline bool mlp_input_affine_ok(float x_scale, float x_shift) {
  return x_scale > 0.f && x_scale <= FLT_MAX && x_shift >= -FLT_MAX && x_shift <= FLT_MAX;  // NaN fails every test
}

struct MLPStepArgs {
  // input: either a uint8 dataset gathered through `order` (GPU-resident data,
  // pixels mapped by fmaf(u8, x_scale, x_shift) in-kernel) or a dense fp32 batch [B, 784].
  const uint8_t* x_u8;      // [N_data, 784] or null
  const float* x_f32;       // [B, 784] or null
  const int64_t* labels;    // [N_data] (u8 mode) or [B] (f32 mode)
  const int64_t* order;     // [n_batches * B] sample indices for the epoch (u8 mode)
  int64_t* counters;        // [0] optimizer step t, [1] batch cursor (u8 mode)
  int64_t n_batches;        // cursor wraps modulo this (u8 mode)
  int B;                    // full batch size (loss is a mean over B)
  int L1, L2;
  float* params;            // arena: W1[L1,784] b1[L1] W2[L2,L1] b2[L2] W3[10,L2] b3[10]
  float* grads;             // same layout
  float* exp_avg;           // Adam state (same layout) when apply_adam
  float* exp_avg_sq;
  float* stats;             // ring [ring, 4]: loss, correct, count, step
  int stats_ring;
  int accumulate_grad;      // add existing grads (gradient accumulation)
  int apply_adam;           // fuse Adam into the gradient epilogues (world size 1)
  int advance_step;         // increment counters[0] (this call completes an optimizer step)
  float lr, beta1, beta2, eps, weight_decay;
  const float* lr_ptr;
  int adamw;
  int64_t* stamps;          // optional [16] phase timestamps (diagnostics)
  // v2 (two-kernel) step only:
  uint16_t* shadow;         // bf16 weight shadows (row-major copy + W2^T + W3^T), see mlp_shadow_layout
  uint16_t* dh1t;           // scratch [L1, round_up(B, 32)] bf16: dH1^T handed from head to W1 kernel
  float x_scale, x_shift;   // u8 mode: pixel = fmaf(u8, x_scale, x_shift) (x_f32 mode ignores them)
};

// bf16 shadow layout (elements): [0, np) row-major copy of the fp32 arena,
// [w2t, w2t + L1*L2) W2^T [L1][L2], [w3t, w3t + 16*L2) W3^T [L2][16] (classes
// zero-padded to 16).  The forward/backward read 16-byte bf16 fragments from it.
struct MLPShadowLayout {
  int64_t np, w2t, w3t, total;
};
MLPShadowLayout mlp_shadow_layout(int L1, int L2);

struct MLPAdamArgs {
  float* params;
  const float* grads;
  float* exp_avg;
  float* exp_avg_sq;
  uint16_t* shadow;
  int L1, L2;
  float lr, beta1, beta2, eps, weight_decay, grad_scale;
  int adamw;
  int update;               // 0: only refresh the shadows from params
  const int64_t* step_ptr;  // already-incremented step
  const float* lr_ptr;
};

struct MLPEvalArgs {
  const uint8_t* x_u8;
  const float* x_f32;
  const int64_t* labels;
  const int64_t* index;     // [B] sample indices (u8 mode) or null
  int B, L1, L2;
  const float* params;
  float* logits;            // optional [B, 10] output (log-probabilities)
  float* out;               // [2]: += sum of NLL, += correct count
                            // (partials: [ceil(B/32), 2] per-32-row-chunk sums, overwritten)
  int partials;
  float x_scale, x_shift;   // u8 mode: pixel = fmaf(u8, x_scale, x_shift) (x_f32 mode ignores them)
};

// v3 (cross-step pipelined layer 1, resident uint8 dataset only); see mlp_step3.hip.
struct MLP3Args {
  const uint8_t* x_u8;      // [N_data, 784]
  const int64_t* labels;    // [N_data]
  const int64_t* order;     // [2][order_stride]: two epochs' sample orders
  int64_t order_stride;     // n_batches * B
  int64_t* counters;        // [10]: (step, next cursor, consumed cursor, ring slot, order buffer) x {current, next};
                            // [10] launch sequence number of the one-launch step (counters of >= 16)
  int64_t n_batches;
  int B, L1, L2;
  // valid rows of the epoch's LAST batch (cursor n_batches - 1), in [1, B]; B: no short batch.
  // Two-launch family and PRIME only (the one-launch and exchange kinds never read it).  It
  // sits in the four bytes of padding the struct always had here, so every other field keeps
  // its kernarg offset and the struct its size.
  int last_rows;
  float* params;
  float* grads;
  float* exp_avg;
  float* exp_avg_sq;
  uint16_t* shadow;         // bf16 weight shadows (mlp_shadow_layout)
  uint16_t* dh1t;           // [L1][Bp] bf16
  uint16_t* xring;          // [2][49][Bp][16] bf16 X tiles
  int* h1pre;               // [2][copies][Bp * L1] layer-1 pre-activations, 12.20 fixed point (fragment order)
  uint16_t* act;            // [L1 + 2*L2 + 16][Bp] bf16 head -> tail: H1^T, H2^T, dH2^T, dZ^T
  int* yring;               // [2][Bp] int32 staged labels (-1 past B), slot-indexed like xring
  float* stats;
  int stats_ring;
  float* head_part;         // [ceil(B/32)][4] per-head-block (sum NLL, #correct, #rows); B > 32
  int apply_adam;           // head: Adam on the small parameters (world size 1)
  int advance_step;
  float lr, beta1, beta2, eps, weight_decay, grad_scale;
  const float* lr_ptr;
  int adamw;
  // the device learning rate is a ring of lr_mask + 1 floats (a power of two) behind lr_ptr:
  // a launch that applies the optimizer for optimizer step t (1-based, Adam's bias-correction
  // count; SGD: the counter behind its first-step rule) reads lr_ptr[(t - 1) & lr_mask].  0:
  // the single scalar lr_ptr[0].  Nothing on the device writes the ring, so a captured graph
  // replays correctly at any step.  Launches that apply no optimizer ignore it.  Like
  // last_rows it sits in four bytes of padding the struct always had (between adamw and
  // stamps): appended after x_shift it would grow the struct and move the hidden kernel
  // arguments of every instance; here no field, no hidden argument and no size changes.
  int lr_mask;
  int64_t* stamps;
  // fused data-parallel tail (kMLP3StepDP): the comm engine's auxiliary peer
  // region (csrc/comm/communicator.h aux_context)
  char* dp_regions[8];
  uint32_t* dp_gen;         // [128] per-block generations (local device memory)
  int* dp_err;              // host-mapped error word
  int64_t dp_stride;        // floats per (slot, rank) receive area (>= param count)
  int64_t dp_spin;          // poll bound
  int dp_rank, dp_world;
  int dp_lite;              // exchange protocol: 2 tagged granules (default), 1 flags + one fencing wave, 0 flags + all waves
  // one-launch step (kMLP3Step1DP) exchange: 0 arena-indexed {gen, fp32} granules (round 2),
  // 1 "packed" one-shot (wave-positioned, two values per granule), 2 "owner" (reduce-scatter to
  // the task's owner rank, Adam there, all-gather of the fp32 weights)
  int dp_proto;
  // loopback (diagnostic): one process plays all dp_world ranks through its own region
  // (kMLP3Step1DP's packed / owner protocols, and kMLP3StepDP under a rate ring, lr_mask != 0:
  // the tail's loopback is compiled into its ring instances; without a ring StepDP refuses it, -3)
  // (every region pointer is this rank's; the block writes every source slot itself)
  int dp_loop;
  // one-launch step (kMLP3Step1): in-launch hand-off words (mlp_step3.hip) and their poll bound.
  // Every kind that computes layer-1 partials (both step forms, the ADAM tail, PRIME) also
  // counts the partials its 12.20 conversion clamped (finite, beyond +-32) or that were NaN /
  // Inf into words sat / nonfinite of this buffer, and the latest affected optimizer step
  // into last_step (mlp3_hand_layout); nullptr (two-launch kinds only): nothing is counted.
  unsigned long long* hand;
  int64_t hand_spin;
  // pixel = fmaf(u8, x_scale, x_shift) wherever a kernel gathers a batch (appended: every
  // other field keeps its kernarg offset)
  float x_scale, x_shift;
};
static_assert(offsetof(MLP3Args, params) == 64 && offsetof(MLP3Args, last_rows) == 60,
              "last_rows fills the padding in front of params");
static_assert(offsetof(MLP3Args, lr_mask) == offsetof(MLP3Args, adamw) + 4 &&
                  offsetof(MLP3Args, stamps) == offsetof(MLP3Args, adamw) + 8 && sizeof(MLP3Args) == 368,
              "lr_mask fills the padding behind adamw");
enum MLP3Kind { kMLP3Step = 0, kMLP3Head = 1, kMLP3TailGrad = 2, kMLP3TailAdam = 3, kMLP3Prime = 4,
                kMLP3StepDP = 5, kMLP3Step1 = 6, kMLP3Step1DP = 7, kMLP3TailAcc = 8 };
int64_t mlp3_hand_words(int L1, int L2);  // int64 words of the one-launch step's hand-off buffer
// word indices of `hand`: ack / err (the one-launch hand-off), sat / nonfinite / last_step
// (exact, monotonic u64 health counts of the layer-1 partial sums)
struct MLP3HandLayout {
  int ack, err, sat, nonfinite, last_step, words;
};
MLP3HandLayout mlp3_hand_layout();
// further words of `hand`: the one-launch step's cache of Adam's bias corrections for the
// next step -- key (step, bits(beta1) | bits(beta2) << 32), 1 - beta1^step and
// sqrt(1 - beta2^step) as f64 bits (mlp_step3.hip)
struct MLP3AdamCacheLayout {
  int step, betas, bc1, bc2_sqrt;
};
MLP3AdamCacheLayout mlp3_adam_cache_layout();
// Global-norm gradient clipping of the ADAM tail (kMLP3TailAdam only): its own kernel
// argument, so MLP3Args and every other kind's launch stay as they are.  `part` holds
// launch_clip_partials' per-block sums of squares over the gradient arena; each block's
// scalar lane sums them in index order and derives
//   norm = sqrt(sum) * grad_scale,  coef = min(1, max_norm / (norm + 1e-6))
// (torch.nn.utils.clip_grad_norm_), and the Adam epilogues read grads * grad_scale * coef.
// `out` (optional, [4] fp32, written by block 0 alone): [0] norm, [1] coef,
// [2] += 1 when coef < 1, [3] += 1 when the norm is NaN / Inf.  part == nullptr: no clipping.
struct MLP3Clip {
  const float* part;
  int nblk;
  float max_norm;
  float* out;
};
constexpr int kClipMaxBlocks = 64;
// Gradient accumulation (kMLP3TailGrad / kMLP3TailAcc only): its own kernel argument, as
// MLP3Clip.  A window of K micro-batches ends in one optimizer step; every micro-batch but
// the last runs head -> TailAcc (gradients, no Adam, the next batch's layer-1 partial from
// the unchanged weights), the last head -> TailGrad -> ... -> TailAdam.
//   add       grads += this micro-batch's gradient (one fp32 add per element) instead of the
//             overwrite; the first micro-batch of a window overwrites, so nothing zero-fills.
//   rows      one stats row per MICRO-batch: the tail writes the row at
//             counters[kMLP3RowWord] % stats_ring and advances that word (the optimizer step
//             no longer identifies a row); column 3 is the optimizer step the batch feeds.
//   head_row  [4] fp32, with `rows` and B <= 32: where this micro-batch's one-block head left
//             its row (the head launch was given it as a one-row `stats`).
// All zero / nullptr: the launches as they were.
struct MLP3Acc {
  int add;
  int rows;
  const float* head_row;
};
constexpr int kMLP3RowWord = 11;  // counters word: stats rows written under MLP3Acc::rows
// SGD instead of Adam in the tail (kMLP3Step / kMLP3TailAdam only; torch.optim.SGD's
// semantics, mlp_common.h sgd1): its own compile-time instances of the tail kernel, which take
// this struct as their last kernel argument -- in the slot where the Adam instances take
// MLP3Acc, so those keep their argument offsets.  The velocity lives behind
// MLP3Args::exp_avg (neither read nor written when momentum == 0); exp_avg_sq is never
// touched and may be null.  lr / weight_decay / grad_scale / lr_ptr are MLP3Args'; the first
// optimizer step (counters[0] <= 1 after the head's advance) sets the velocity to the gradient.
// enabled == 0: Adam, the launches as they were.
struct MLP3Sgd {
  int enabled;
  float momentum, dampening;
  int nesterov;
};
// Returns 0, or a negative code before any launch: -8 misplaced clip arguments, -10 MLP3Acc
// flags on a kind other than TailGrad / TailAcc (or rows without a row source), -11 TailAcc
// with clip arguments, -12 MLP3Sgd on a kind other than Step / TailAdam (or momentum without
// a velocity buffer), -13 a non-finite or non-positive x_scale or a non-finite x_shift, -14
// Step1DP with a pixel map other than the default (StepDP serves a normalised dataset), -15
// last_rows outside [1, B], or last_rows != B on Step1 / Step1DP / StepDP (a short last batch
// runs on the two-launch family: Head, Step, TailGrad, TailAcc, TailAdam, and on PRIME), -16
// Step1DP with lr_mask != 0 (the one-launch exchange has no schedule instance: StepDP serves
// a rate ring, as it serves a normalised dataset), -17 an lr_mask that is not 2^k - 1, or one
// without lr_ptr.
int launch_mlp3(const MLP3Args& a, int kind, hipStream_t stream, const MLP3Clip* clip = nullptr,
                const MLP3Acc* acc = nullptr, const MLP3Sgd* sgd = nullptr);

int mlp3_act_rows(int L1, int L2);
int mlp3_h1_copies(int L1);  // H1pre copies per ring slot (mlp_step3.hip H1Copies)
// the packed DP exchange's wire form of fp32 pairs, encoded and decoded (tests)
int dp_pack_roundtrip(const float* x, float* y, int64_t n, int tag, hipStream_t stream);

// returns 0 on success, -1 if (L1, L2) has no compiled instantiation, -13 (before any launch,
// u8 mode) for a non-finite or non-positive x_scale or a non-finite x_shift
int launch_mlp_train_step(const MLPStepArgs& a, hipStream_t stream);
int launch_mlp_eval(const MLPEvalArgs& a, hipStream_t stream);
bool mlp_supported(int L1, int L2);
int launch_mlp_adam(const MLPAdamArgs& a, hipStream_t stream);

}  // namespace rla

namespace rla {
// ---------------------------------------------------------------------------
// Weight gradient of NHWC bf16 convolutions on MFMA (csrc/conv_wgrad.hip):
// dW [Cout][KH][KW][Cin] fp32 = sum over output rows of dy x shifted x.
// Cout % 64 == 0, Cin % 64 == 0.
// ---------------------------------------------------------------------------
struct WgradGeom {
  int N, H, W, Cin;   // x  [N, H, W, Cin]
  int OH, OW, Cout;   // dy [N, OH, OW, Cout]
  int KH, KW, sh, sw, ph, pw;
};
struct WgradPlan {
  int kind;                // 0 generic (any geometry), 1 3x3 / stride 1 / pad 1 halo kernel
  int wa, wb;              // workgroup tile = (64 wa) x (64 wb) channels
  int splits;              // row splits (> 1: fp32 partials + a reduce kernel)
  int64_t rows_per_split;  // kind 1: stages (64 output rows each) per split
};
// splits <= 0: automatic; algo 0: the halo kernel when the geometry allows, 1: generic
WgradPlan wgrad_plan(const WgradGeom& g, int splits, int algo = 0);
// part: splits * Cout * KH * KW * Cin floats when plan.splits > 1 (else unused)
// pre_ss ([4, Cin] BatchNorm stats; every plan: the generic kernel at any filter, stride and
// padding, and the halo kernel): x is a deferred BatchNorm + ReLU's input, staged as
// bf16(relu(x * scale + shift)) inside the image; zero-padding taps stay zero
void launch_wgrad(const uint16_t* dy, const uint16_t* x, float* out, float* part, const WgradGeom& g,
                  const WgradPlan& p, hipStream_t stream, const float* pre_ss = nullptr);

// ---------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 NHWC bf16 convolution on MFMA (csrc/conv3x3.hip):
// y [N, H, W, Cout] = conv(x [N, H, W, Cin], w [Cout][3][3][Cin]); also the input
// gradient with the flipped, transposed weight.  Cin % 16 == 0, Cout % 64 == 0.
// ---------------------------------------------------------------------------
struct Conv3x3Geom {
  int N, H, W, Cin, Cout;
  int vrows;  // halo rows of the largest pixel tile (conv3x3_vrows)
  int tm;     // pixels per workgroup tile: 256 or 512 (conv3x3_pick_tm)
  int wpb;    // workgroups per 64-channel output block = contiguous pixel ranges (conv3x3_wpb)
};
// The CU count the persistent kernels' work splits are planned for (conv3x3_wpb,
// conv1x1_stats_plan, stem_grid): the device's, unless set_plan_cus(n > 0) pinned one
// for the whole process (n <= 0 restores the device value).  Read on every plan call.
int plan_cus();
void set_plan_cus(int n);
int conv3x3_wpb(int N, int H, int W, int Cout);
int conv3x3_pick_tm(int N, int H, int W, int Cout);
int conv3x3_vrows(const Conv3x3Geom& g);
// The arguments a 3x3 geometry of either stride can be built from: all positive, the pixel
// and channel counts in int range (N (H + 2) (W + 2), Cin, Cout < 2^30) and Cout % 64 == 0,
// which conv3x3_wpb divides by.
bool conv3x3_args_ok(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout);
// The one cache of the partition walks (conv3x3_vrows, conv3x3s2_vrows and, under stride key
// 3, conv3x3s2_dgrad_vrows), keyed on all a
// walk's answer is a function of; a pinned plan CU count or RLA_CONV3X3_TM changes tm / wpb,
// hence the key.  walk() runs on a key's first use.
int conv3x3_cached_vrows(int stride, int N, int H, int W, int tm, int wpb, const std::function<int()>& walk);
// The geometry of every stride-1 launch, predicate and plan query, under the current
// plan_cus() and RLA_CONV3X3_TM.  Guards conv3x3_args_ok (what makes the int casts and the
// planning arithmetic safe): arguments that fail it give the all-zero geometry, which
// conv3x3_ok refuses.  Cin % 16, the halo limit and the 32-bit offset limits are conv3x3_ok's.
Conv3x3Geom conv3x3_geom(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout);
int conv3x3_pieces_per_thread(const Conv3x3Geom& g);  // 16-byte halo pieces per thread and chunk
bool conv3x3_ok(const Conv3x3Geom& g);
// the template instance launch_conv3x3 runs for g (pre: with pre_ss; with bwd_x: that of pre = false)
struct Conv3x3Instance {
  int nx;      // halo pieces per thread the instance is compiled for
  bool fixed;  // compile-time width and input channels
};
Conv3x3Instance conv3x3_instance(const Conv3x3Geom& g, bool pre);
// flip: input gradient -- x is dy [N, H, W, Cin], w the FORWARD weight [Cin][3][3][Cout]
// (Cin = the forward's output channels), y is dx [N, H, W, Cout]
// part (forward only, or null): BatchNorm partial sums of bf16(y), [g.wpb][2][Cout] fp32
// pre_ss (forward with part only; [4, Cin] BatchNorm stats, Cin <= 512): x is a deferred
// BatchNorm + ReLU's input, staged as bf16(relu(x * scale + shift)); nbt_inc += 1
// bwd_x (flip with part and pre_ss only; Cout <= 512): the PRECEDING BatchNorm + ReLU's
// backward in the epilogue -- bwd_x [N, H, W, Cout] is that BatchNorm's input, pre_ss its
// [4, Cout] statistics; y is d = fma(bwd_x, scale, shift) > 0 ? dx : 0 and part
// [g.wpb][2][Cout] the sums of d and d * bwd_x over each range (bn_partial's backward layout)
bool conv3x3_pre_ok(const Conv3x3Geom& g);
bool conv3x3_bwd_ok(const Conv3x3Geom& g);
bool launch_conv3x3(const uint16_t* x, const uint16_t* w, uint16_t* y, const Conv3x3Geom& g, bool flip,
                    hipStream_t stream, float* part = nullptr, const float* pre_ss = nullptr,
                    int64_t* nbt_inc = nullptr, const uint16_t* bwd_x = nullptr);

// 3x3 / stride 2 / pad 1 NHWC bf16 convolution forward on MFMA (csrc/conv3x3s2.hip):
// y [N, OH, OW, Cout] = conv(x [N, H, W, Cin], w [Cout][3][3][Cin]), OH = (H - 1) / 2 + 1,
// OW = (W - 1) / 2 + 1.  Cin % 16 == 0, Cout % 64 == 0.
struct Conv3x3S2Geom {
  int N, H, W, Cin, Cout, OH, OW;
  int vrows;  // halo rows of the largest pixel tile (conv3x3s2_vrows)
  int wpb;    // workgroups per 64-channel output block = contiguous output-pixel ranges
};
// conv3x3_geom's stride-2 counterpart, with the same guard and the same all-zero answer
// (wpb = conv3x3_wpb over the OUTPUT pixels); Cin % 16 and the halo limit are conv3x3s2_ok's
Conv3x3S2Geom conv3x3s2_geom(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout);
int conv3x3s2_vrows(const Conv3x3S2Geom& g);
int conv3x3s2_pieces_per_thread(const Conv3x3S2Geom& g);  // 16-byte halo pieces per thread and chunk
int conv3x3s2_tm();  // output pixels per workgroup tile
int conv3x3s2_nx();  // halo pieces per thread the kernel is compiled for
bool conv3x3s2_ok(const Conv3x3S2Geom& g);
// part (or null): BatchNorm partial sums of bf16(y), [g.wpb][2][Cout] fp32
bool launch_conv3x3s2(const uint16_t* x, const uint16_t* w, uint16_t* y, const Conv3x3S2Geom& g,
                      hipStream_t stream, float* part = nullptr);

// Input gradient of the 3x3 / stride 2 / pad 1 convolution on MFMA (csrc/conv3x3s2_dgrad.hip):
// dx [N, H, W, Co] from dy [N, OH, OW, Cr] and the FORWARD weight w [Cr][3][3][Co] (Cr the
// layer's output channels, Co its input channels, as conv3x3_dgrad_bn names them).  The work
// is tiled over quads (n, a, b), a < OH, b < OW: the input pixels (2 a + {0, 1}, 2 b + {0, 1}).
// Cr % 16 == 0, Co % 64 == 0.
struct Conv3x3S2DgradGeom {
  int N, H, W, Cr, Co, OH, OW;
  int vrows;  // dy halo rows of the largest quad tile (conv3x3s2_dgrad_vrows)
  int wpb;    // workgroups per 64-channel dx block = contiguous quad ranges
};
// conv3x3s2_geom's counterpart, with the same guard and the same all-zero answer
// (wpb = conv3x3_wpb over the quads); Cr % 16 and the halo limit are conv3x3s2_dgrad_ok's
Conv3x3S2DgradGeom conv3x3s2_dgrad_geom(int64_t N, int64_t H, int64_t W, int64_t Cr, int64_t Co);
int conv3x3s2_dgrad_vrows(const Conv3x3S2DgradGeom& g);
int conv3x3s2_dgrad_pieces_per_thread(const Conv3x3S2DgradGeom& g);  // 16-byte halo pieces per thread and chunk
int conv3x3s2_dgrad_tq();  // quads per workgroup tile
int conv3x3s2_dgrad_nx(const Conv3x3S2DgradGeom& g);  // halo pieces per thread of the instance g runs (2, 3 or 4)
bool conv3x3s2_dgrad_ok(const Conv3x3S2DgradGeom& g);
bool launch_conv3x3s2_dgrad(const uint16_t* dy, const uint16_t* w, uint16_t* dx, const Conv3x3S2DgradGeom& g,
                            hipStream_t stream);

// ResNet stem: 7x7 / stride 2 / pad 3 convolution, 3 -> 64 channels, NHWC bf16 (csrc/stem.hip);
// part (or null): BatchNorm partial sums of bf16(y), [stem_grid(g)][2][64] fp32
struct StemGeom {
  int N, H, W, OH, OW;
};
// guards the int casts only (out-of-range sizes give the all-zero geometry); the shapes the
// kernels cover are stem_ok's
StemGeom stem_geom(int64_t N, int64_t H, int64_t W);
bool stem_ok(const StemGeom& g);
int stem_grid(const StemGeom& g);
bool launch_stem_fwd(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, const StemGeom& g,
                     hipStream_t stream);
// weight gradient: dy [N, OH, OW, 64] bf16 -> dw [64][7][7][3] fp32; part: [stem_grid(g)][64][224] fp32 workspace
bool launch_stem_wgrad(const uint16_t* x, const uint16_t* dy, float* part, float* dw, const StemGeom& g,
                       hipStream_t stream);

}  // namespace rla
