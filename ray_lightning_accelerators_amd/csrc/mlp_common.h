// Shared pieces of the fused MNIST-MLP kernels (mlp_step3.hip step, mlp_adam.hip
// arena Adam): arena offsets, Adam scalar math, LDS fragment loaders.
#pragma once
#include <math.h>

#include "common.h"

namespace rla {
namespace mlp {

constexpr int kD = 784;   // input features
constexpr int kNC = 10;   // classes
constexpr int kTiles = kD / 16;  // 16-pixel W1 column tiles (49)

// fp32 arena == bf16 shadow row-major copy; W2^T / W3^T follow in the shadow.
template <int L1, int L2>
struct Off {
  static constexpr int64_t W1 = 0, B1 = (int64_t)L1 * kD, W2 = B1 + L1, B2 = W2 + (int64_t)L2 * L1,
                           W3 = B2 + L2, B3 = W3 + kNC * L2, NP = B3 + kNC;
  static constexpr int64_t W2T = (NP + 7) / 8 * 8, W3T = W2T + (int64_t)L1 * L2;
};

struct AdamScal {
  float lr, step_size, bc2_sqrt, beta1, beta2, eps, wd;
  int adamw;
};

// torch.optim.Adam's bias corrections, in double like the eager optimizer.
__device__ __forceinline__ void adam_scalars(AdamScal& o, int64_t t, float lr, float b1, float b2, float eps,
                                             float wd, int adamw) {
  const double bc1 = 1.0 - pow((double)b1, (double)t);
  const double bc2 = 1.0 - pow((double)b2, (double)t);
  o.lr = lr;
  o.step_size = (float)((double)lr / bc1);
  o.bc2_sqrt = (float)sqrt(bc2);
  o.beta1 = b1; o.beta2 = b2; o.eps = eps; o.wd = wd; o.adamw = adamw;
}

// The part of adam_scalars that depends on (t, beta1, beta2) only -- the two pow() --
// as the one-launch step caches it from one step to the next (mlp_step3.hip, "Adam
// bias-correction cache"): bc1 = 1 - beta1^t and sqrt(1 - beta2^t), both in double.
struct AdamBias {
  double bc1, bc2_sqrt;
};

// Both powers in ONE instruction stream: lane 0 of the wave evaluates pow(beta1, t),
// lane 1 pow(beta2, t) (one pow()'s dependent chain where adam_scalars has two),
// and every calling lane receives both through readlane (no LDS round trip).  Each
// lane runs the same pow() on the same arguments as adam_scalars, so the bits are
// adam_scalars' bits.  Call with (at least) lanes 0 and 1 of the wave active.
__device__ __forceinline__ AdamBias adam_bias2(int64_t t, float b1, float b2) {
  const bool first = (threadIdx.x & 63) == 0;
  const double p = pow((double)(first ? b1 : b2), (double)t);
  const int lo = __double2loint(p), hi = __double2hiint(p);
  const double p1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
  const double p2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 1), __builtin_amdgcn_readlane(lo, 1));
  return AdamBias{1.0 - p1, sqrt(1.0 - p2)};
}

// adam_scalars with the bias corrections given: the learning rate is applied here
// (it may change between any two steps), the same operations on the same doubles.
__device__ __forceinline__ void adam_scalars_bias(AdamScal& o, const AdamBias& c, float lr, float b1, float b2,
                                                  float eps, float wd, int adamw) {
  o.lr = lr;
  o.step_size = (float)((double)lr / c.bc1);
  o.bc2_sqrt = (float)c.bc2_sqrt;
  o.beta1 = b1; o.beta2 = b2; o.eps = eps; o.wd = wd; o.adamw = adamw;
}

// Explicit FMAs and no compiler contraction: every kernel that inlines this (tail
// epilogues, the one-launch step's tiles, the arena Adam) computes the same bits.
__device__ __forceinline__ float adam1(float p, float g, float& m, float& v, const AdamScal& o) {
#pragma clang fp contract(off)
  if (o.wd != 0.f) {
    if (o.adamw) p = p * (1.f - o.lr * o.wd);
    else g = fmaf(o.wd, p, g);
  }
  m = fmaf(1.f - o.beta1, g - m, m);
  v = fmaf(1.f - o.beta2, g * g, v * o.beta2);
  const float denom = sqrtf(v) / o.bc2_sqrt + o.eps;
  return fmaf(-o.step_size, m / denom, p);
}

// torch.optim.SGD's per-step scalars.  `first`: the launch belongs to optimizer step
// t <= 1, where the velocity is the gradient itself (optim_kernels.hip sgd_kernel's rule).
struct SgdScal {
  float lr, momentum, one_minus_damp, wd;
  int nesterov, first;
};

// One SGD element, torch's order of operations; explicit FMAs and no contraction, like
// adam1: the tile epilogue and both small-parameter routes write the same bits.  `buf`
// is neither read nor written when momentum == 0.
__device__ __forceinline__ float sgd1(float p, float g, float& buf, const SgdScal& o) {
#pragma clang fp contract(off)
  if (o.wd != 0.f) g = fmaf(o.wd, p, g);
  if (o.momentum != 0.f) {
    buf = o.first ? g : fmaf(o.momentum, buf, o.one_minus_damp * g);
    g = o.nesterov ? fmaf(o.momentum, buf, g) : buf;
  }
  return fmaf(-o.lr, g, p);
}

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
// ds_read_b64_tr_b16: lane i of each 16-lane group receives column i of the
// 4x16 bf16 block whose rows lanes 4q+p point at.
__device__ __forceinline__ bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p));
}
__device__ __forceinline__ bf16x8 ld8(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// u8 pixels (16 per uint4) -> two bf16x8, scaled by 1/255 (torchvision ToTensor).
__device__ __forceinline__ void u8x16_to_bf16(const uint4 v, bf16x8& lo, bf16x8& hi) {
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
  constexpr float inv255 = 1.0f / 255.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (__bf16)((float)((wd[0] >> (8 * j)) & 0xffu) * inv255);
    lo[4 + j] = (__bf16)((float)((wd[1] >> (8 * j)) & 0xffu) * inv255);
    hi[j] = (__bf16)((float)((wd[2] >> (8 * j)) & 0xffu) * inv255);
    hi[4 + j] = (__bf16)((float)((wd[3] >> (8 * j)) & 0xffu) * inv255);
  }
}

// The same with the pixel map as two run-time scalars: bf16(fmaf(u8, x_scale, x_shift)) --
// ToTensor (x_scale = 1/255, x_shift = 0: bitwise the product above for every byte) with an
// optional single-channel Normalize folded in (kernels.h kMLPXScale).
__device__ __forceinline__ void u8x16_to_bf16(const uint4 v, bf16x8& lo, bf16x8& hi, float x_scale,
                                              float x_shift) {
  const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (__bf16)fmaf((float)((wd[0] >> (8 * j)) & 0xffu), x_scale, x_shift);
    lo[4 + j] = (__bf16)fmaf((float)((wd[1] >> (8 * j)) & 0xffu), x_scale, x_shift);
    hi[j] = (__bf16)fmaf((float)((wd[2] >> (8 * j)) & 0xffu), x_scale, x_shift);
    hi[4 + j] = (__bf16)fmaf((float)((wd[3] >> (8 * j)) & 0xffu), x_scale, x_shift);
  }
}

}  // namespace mlp
}  // namespace rla
