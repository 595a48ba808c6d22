// Last launch of the multi-workgroup MNIST steps (mlp_step_wide.hip, mlp_step_general.hip):
// slices summed in slice order, the epilogue, the stats row and the counters.  Width-agnostic:
// one thread per parameter of the flat arena.  Included by both files, so each keeps a copy of
// the one kernel in its own translation unit.
#pragma once
#include "common.h"
#include "kernels.h"
#include "mlp_common.h"

namespace rla {
namespace {

constexpr int kApplyThreads = 256;

__global__ __launch_bounds__(kApplyThreads) void mlp_wide_apply_kernel(MLPWideArgs w, int64_t np, int S, int nslab) {
  using namespace mlp;
  const MLPStepArgs& a = w.step;
  __shared__ AdamScal sh_o;
  const int64_t t = w.hdr[0];
  if (a.apply_adam && threadIdx.x == 0) {
    const float lr = a.lr_ptr ? a.lr_ptr[(t - 1) & w.lr_mask] : a.lr;
    adam_scalars(sh_o, t, lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.adamw);
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kApplyThreads + threadIdx.x;
  if (i < np) {
    float gsum = w.part[i];
    for (int s = 1; s < S; ++s) gsum += w.part[(int64_t)s * w.np_pad + i];
    if (a.accumulate_grad) gsum += a.grads[i];
    if (a.apply_adam) {
      float m = a.exp_avg[i], v = a.exp_avg_sq[i];
      a.params[i] = adam1(a.params[i], gsum, m, v, sh_o);
      a.exp_avg[i] = m;
      a.exp_avg_sq[i] = v;
    } else {
      a.grads[i] = gsum;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t cursor = w.hdr[1];
    if (a.counters) {
      if (a.advance_step) a.counters[0] = t;
      if (a.x_u8) a.counters[1] = (a.n_batches > 0) ? (cursor + 1) % a.n_batches : cursor + 1;
    }
    if (a.stats) {
      float loss = 0.f, hit = 0.f, cnt = 0.f;
      for (int sl = 0; sl < nslab; ++sl) {
        loss += w.slab_stats[sl * 4];
        hit += w.slab_stats[sl * 4 + 1];
        cnt += w.slab_stats[sl * 4 + 2];
      }
      float* st = a.stats + ((t - 1) % (a.stats_ring > 0 ? a.stats_ring : 1)) * 4;
      st[0] = loss * (1.f / (float)w.hdr[2]);
      st[1] = hit;
      st[2] = cnt;
      st[3] = (float)t;
    }
  }
}

}  // namespace
}  // namespace rla
