// 1x1 / stride-1 NHWC bf16 convolution forward with the following BatchNorm's batch
// statistics in its epilogue, for LONG K and FEW tiles (gfx950): the contract of
// conv1x1.hip's conv1x1_stats_kernel,
//
//   y[m][n] = bf16(sum_k x[m][k] * w[n][k])
//   part[b][0][n] = sum over pixel range b of bf16(y[m][n]),  part[b][1][n] = of its square
//
// with another work split.  conv1x1.hip loses the K >= 256 ResNet-50 layers to the
// library: its 128 x 128 tiles at 32-channel stages re-read x through L2 once per
// 128-channel column, and the 14x14 / 7x7 layers have too few tiles for 256 CUs
// (docs/resnet50.md).  Here:
//   * ONE 512-thread workgroup per CU (8 waves = 2 pixel halves x 4 channel quarters)
//     owns 128 pixels x BN channels, BN = 256 (a wave: 64 x 64 = 2 x 2 blocks of
//     v_mfma_f32_32x32x16_bf16, 64 accumulators) or 128 (64 x 32).  With BN = 256 and
//     N <= 256 every x row is fetched once; only the weight block streams from L2;
//   * a K-stage is 64 channels: x [8 k units][128 rows] and w [8 k units][BN rows] of
//     16 B, unit-major as in conv1x1.hip (fragment reads are contiguous 512-B
//     ds_read_b128 runs), both by LDS-DMA into a ring of 3 stages of 48 KB (BN = 256)
//     or 4 of 32 KB (BN = 128); a stage is retired by a counted vmcnt and one raw
//     barrier, across tile boundaries (the DMA is inline asm the compiler's wait
//     bookkeeping does not see; the loop holds no other load);
//   * pixel ranges are persistent (`tiles_per_blk` consecutive tiles, statistics carried
//     in registers) and dealt XCD-aware: hardware block b runs on XCD b % 8, and all
//     channel columns and K-slices of a pixel range sit on one XCD;
//   * deterministic split-K where the tiles cannot fill the machine (S = 2 / 4 slices of
//     whole stages, only with one tile per workgroup): every slice stores its fp32
//     accumulators to ws[tile][slice][128 x BN] in lane-native order (16-byte stores)
//     and takes a ticket from counter[tile] (acq_rel, agent scope); the workgroup that
//     draws S - 1 loads ALL S slices back, its own included, adds them in slice order
//     and runs the epilogue -- the result does not depend on which slice arrives last
//     nor on where the slices ran.  Nobody waits for anybody: no spin, no grid barrier.
//     The finisher sets the counter back to 0 (the binding zeroes fresh counters per call
//     and does not rely on it; a caller that keeps its counters may).  Measured, the slices
//     never pay (docs/resnet50.md): the planner leaves splits at 1 and the instances run
//     only when asked for (conv1x1_wide_plan).
// Epilogue (conv1x1.hip's): round to bf16, add the ROUNDED values into the lane's
// per-channel sums, one v_permlane32_swap per dword pair widens the stores to 16 bytes;
// at the end a butterfly over the 32 pixel lanes and a fixed-order LDS add over the two
// pixel-half waves.  No float atomics.  Rows past M read a clamped row (never stored,
// excluded from the sums); stages past the end re-load the last one, so every iteration
// issues the same DMA count; padding ranges of the XCD deal write zero partial rows.
// Requires K >= 256, K % 64 == 0, N % BN == 0, 16-byte aligned bases (binding checks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "lds_dma.h"

namespace rla {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kCwThreads = 512;
constexpr int kCwTile = 128;  // pixels per tile

template <int BN, bool SPLIT>
__global__ __launch_bounds__(kCwThreads) void conv1x1_wide_kernel(const uint16_t* __restrict__ x,
                                                                  const uint16_t* __restrict__ w,
                                                                  uint16_t* __restrict__ y, int64_t M, int K, int N,
                                                                  int tiles_per_blk, int splits,
                                                                  float* __restrict__ part, float* ws,
                                                                  unsigned* counter) {
  constexpr int TNW = BN / 128;             // 32-channel blocks per wave
  constexpr int NS = BN == 256 ? 3 : 4;     // ring depth
  constexpr int kXBytes = 8 * kCwTile * 16;  // x part of a stage: [8 k units][128 rows] x 16 B
  constexpr int kStageBytes = kXBytes + 8 * BN * 16;
  constexpr int kXInst = 2, kWInst = BN / 64;  // DMA instructions per wave per stage
  constexpr int kDma = kXInst + kWInst;
  static_assert(NS * kStageBytes + 4 * BN * 4 + 16 <= 160 * 1024, "LDS budget (one workgroup per CU)");
  __shared__ __attribute__((aligned(16))) uint8_t ring[NS * kStageBytes];
  __shared__ float red[2][2][BN];
  __shared__ unsigned ticket;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 3, wm = wave >> 2, r = lane & 31, h = lane >> 5;
  const int S = SPLIT ? splits : 1;
  // XCD-aware deal: the gy columns x S slices of pixel range bx all sit on XCD bx % 8
  // (gx is a multiple of 8); only locality depends on it
  const int gy = N / BN, per = gy * S;
  const int xcd = (int)(blockIdx.x % 8u), slot = (int)(blockIdx.x / 8u);
  const int bx = xcd + 8 * (slot / per), by = (slot % per) / S, ks = slot % S;
  const int mt = (int)((M + kCwTile - 1) / kCwTile);
  const int t0 = bx * tiles_per_blk;
  const int ntiles = mt - t0 < tiles_per_blk ? mt - t0 : tiles_per_blk;
  const int nb = by * BN;  // workgroup's first channel
  float* prow = part + (int64_t)bx * 2 * N + nb;
  if (ntiles <= 0) {  // padding range of the XCD deal: an all-zero partial row
    if (ks == 0)
      for (int c = tid; c < BN; c += kCwThreads) {
        prow[c] = 0.f;
        prow[N + c] = 0.f;
      }
    return;
  }
  // this workgroup's K-slice: whole 64-channel stages, the first nstg % S slices one longer
  const int nstg = K >> 6, sb = nstg / S, sr = nstg % S;
  const int nch = sb + (ks < sr ? 1 : 0);
  const int k0 = (ks * sb + (ks < sr ? ks : sr)) * 64;
  const int nst = ntiles * nch;
  const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)ring;

  // DMA of stage st into ring buffer st % NS: wave-instruction g of the x part covers
  // k unit g / 2, rows 64 (g & 1) .. +64; of the w part k unit g / (BN / 64)
  auto issue = [&](int st) {
    const int sc = st < nst ? st : nst - 1;
    const int ti = sc / nch, k = k0 + (sc - ti * nch) * 64;
    const uint32_t buf = ring0 + (uint32_t)(st % NS) * kStageBytes;
#pragma unroll
    for (int u = 0; u < kXInst; ++u) {
      const int g = wave * kXInst + u;
      int64_t m = (int64_t)(t0 + ti) * kCwTile + (g & 1) * 64 + lane;
      m = m < M ? m : M - 1;
      c1_dma16(x + m * K + k + 8 * (g >> 1), __builtin_amdgcn_readfirstlane(buf + g * 1024));
    }
#pragma unroll
    for (int u = 0; u < kWInst; ++u) {
      const int g = wave * kWInst + u;
      const int row = (g % (BN / 64)) * 64 + lane;
      c1_dma16(w + (int64_t)(nb + row) * K + k + 8 * (g / (BN / 64)),
               __builtin_amdgcn_readfirstlane(buf + kXBytes + g * 1024));
    }
  };

  f32x16 acc[TNW][2];
  float ssum[TNW][16], ssq[TNW][16];
#pragma unroll
  for (int t = 0; t < TNW; ++t) {
#pragma unroll
    for (int e = 0; e < 16; ++e) ssum[t][e] = ssq[t][e] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[t][j] = f32x16{};
  }

  // lane l of v_mfma_f32_32x32x16_bf16: row l & 31, k = 8 (l >> 5) .. +8 of both operands
  auto compute = [&](int st) {
    const uint8_t* buf = ring + (st % NS) * kStageBytes;
    const uint8_t* wb = buf + kXBytes;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ku = 2 * s + h;
      bf16x8 fa[TNW], fb[2];
#pragma unroll
      for (int t = 0; t < TNW; ++t)
        fa[t] = *reinterpret_cast<const bf16x8*>(wb + (ku * BN + wn * 32 * TNW + 32 * t + r) * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(buf + (ku * kCwTile + wm * 64 + 32 * j + r) * 16);
#pragma unroll
      for (int t = 0; t < TNW; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t], fb[j], acc[t][j], 0, 0, 0);
    }
  };

  const int cw = nb + wn * 32 * TNW;  // wave's first channel
  // D[n][m]: lane -> pixel r of block j; accumulator 4q + e -> channel 8q + 4h + e.
  // One v_permlane32_swap per dword of each channel-group pair (q, q + 1) gives lane h
  // channels 16p + 8h .. +8: one 16-byte store where the MFMA layout gives two of 8
  auto epilogue = [&](int ti) {
    const int64_t m0 = (int64_t)(t0 + ti) * kCwTile + wm * 64 + r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t m = m0 + 32 * j;
      const bool ok = m < M;  // lanes l and l ^ 32 share the pixel: the swap stays in-pixel
      uint16_t* yo = y + (ok ? m : 0) * N + cw + 8 * h;
#pragma unroll
      for (int t = 0; t < TNW; ++t) {
        uint32_t v[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x4 b;
#pragma unroll
          for (int e = 0; e < 4; ++e) b[e] = (__bf16)acc[t][j][4 * q + e];
          if (ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float f = (float)b[e];
              ssum[t][4 * q + e] += f;
              ssq[t][4 * q + e] += f * f;
            }
          }
          const u32x2 pk = __builtin_bit_cast(u32x2, b);
          v[q][0] = pk[0];
          v[q][1] = pk[1];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(v[2 * p][0], v[2 * p + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(v[2 * p][1], v[2 * p + 1][1], false, false);
          const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
          if (ok) *reinterpret_cast<u32x4*>(yo + 32 * t + 16 * p) = o;
        }
      }
#pragma unroll
      for (int t = 0; t < TNW; ++t) acc[t][j] = f32x16{};
    }
  };

#pragma unroll
  for (int d = 0; d < NS - 1; ++d) issue(d);
  for (int st = 0; st < nst; ++st) {
    // stage st landed: the DMA issued after it (NS - 2 stages) may still fly (an
    // epilogue's stores, younger still, only make the wait longer); then every wave's
    // part is in and every wave has finished reading buffer st - 1
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"((NS - 2) * kDma) : "memory");
    issue(st + NS - 1);
    compute(st);
    if constexpr (!SPLIT) {
      const int ti = st / nch;
      if (st - ti * nch == nch - 1) epilogue(ti);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may outlive the workgroup's LDS

  if constexpr (SPLIT) {
    // one tile per workgroup (t0 = bx < mt): this slice's accumulators to the workspace,
    // thread-linear per 16-byte chunk
    const int64_t tile = (int64_t)bx * gy + by;
    float* slab = ws + tile * S * (kCwTile * BN);
    float* mine = slab + (int64_t)ks * (kCwTile * BN) + tid * 4;
#pragma unroll
    for (int t = 0; t < TNW; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = {acc[t][j][4 * q], acc[t][j][4 * q + 1], acc[t][j][4 * q + 2], acc[t][j][4 * q + 3]};
          *reinterpret_cast<f32x4*>(mine + ((t * 2 + j) * 4 + q) * (kCwThreads * 4)) = v;
        }
    // the barrier orders every wave's stores before thread 0's ticket, whose agent-scope
    // release is cumulative: they are visible to the finisher's loads after its acquire.
    // (The barrier itself carries no vmcnt wait here; each wave drains its own stores into
    // L2 first -- a wait, no cache maintenance -- so the one L2 write-back of thread 0's
    // release finds them all there.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) ticket = __hip_atomic_fetch_add(counter + tile, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (ticket != (unsigned)(S - 1)) return;  // workgroup-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid == 0) __hip_atomic_store(counter + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int t = 0; t < TNW; ++t)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][j] = f32x16{};
    for (int s = 0; s < S; ++s) {  // slice order, whoever finishes
      const float* src = slab + (int64_t)s * (kCwTile * BN) + tid * 4;
#pragma unroll
      for (int t = 0; t < TNW; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(src + ((t * 2 + j) * 4 + q) * (kCwThreads * 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][j][4 * q + e] += v[e];
          }
    }
    epilogue(0);
  }

  // per-channel totals: butterfly over the 32 pixel lanes of each half-wave, then the
  // two pixel-half waves in a fixed order
#pragma unroll
  for (int t = 0; t < TNW; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float a = ssum[t][e], b = ssq[t][e];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
      }
      if (r == 0) {
        const int c = wn * 32 * TNW + 32 * t + 8 * (e >> 2) + 4 * h + (e & 3);
        red[wm][0][c] = a;
        red[wm][1][c] = b;
      }
    }
  __syncthreads();
  for (int c = tid; c < BN; c += kCwThreads) {
    prow[c] = red[0][0][c] + red[1][0][c];
    prow[N + c] = red[0][1][c] + red[1][1][c];
  }
}

}  // namespace

bool conv1x1_wide_ok(int64_t M, int K, int N) {
  return M > 0 && M < (int64_t(1) << 37) && K >= 256 && K % 64 == 0 && N >= 128 && N % 128 == 0 && N <= 4096;
}

Conv1x1WidePlan conv1x1_wide_plan(int64_t M, int K, int N, int bn, int splits) {
  Conv1x1WidePlan p{0, 1, 0, 0};
  if (!conv1x1_wide_ok(M, K, N)) return p;
  const int cus = plan_cus();
  const int64_t mt = (M + kCwTile - 1) / kCwTile;
  // measured per shape (scripts/conv1x1_wide_probe.py, profiles/r22_conv1x1_wide/): 256
  // channels where N allows, but 128 where the 256-wide tiles fill less than half the CUs
  // (6272 x 2048 -> 512: 98 tiles 60 us, 196 tiles 40 us; at 196 of the wide tiles,
  // 25088 x 1024 -> 256, 256 still wins 39.1 to 41.2 us)
  if (bn == 0) bn = N % 256 == 0 && mt * (N / 256) * 2 >= cus ? 256 : 128;
  if ((bn != 256 && bn != 128) || N % bn != 0) return p;
  if (splits != 0 && splits != 1 && splits != 2 && splits != 4) return p;
  const int gy = N / bn;
  // one resident workgroup per CU over the whole grid; gx a multiple of 8 (XCD deal)
  int64_t want = cus / gy;
  if (want < 8) want = 8;
  if (want > mt) want = mt;
  const int64_t tpb = (mt + want - 1) / want;
  const int64_t gx = ((mt + tpb - 1) / tpb + 7) / 8 * 8;
  // a persistent range carries its statistics across tiles: no slices
  if (tpb > 1 && splits > 1) return p;
  p.bn = bn;
  // never sliced unasked: no sliced instance beat the best unsliced one of its shape --
  // 2 slices cost 1.0 - 2.3x the same tile unsliced, 4 slices 1.5 - 3.5x (same sweep)
  p.splits = splits > 1 ? splits : 1;
  p.gx = (int)gx;
  p.tiles_per_blk = (int)tpb;
  return p;
}

int64_t conv1x1_wide_tiles(int64_t M, int N, const Conv1x1WidePlan& p) {
  return p.splits > 1 ? (M + kCwTile - 1) / kCwTile * (N / p.bn) : 0;
}

int64_t conv1x1_wide_ws_floats(int64_t M, int N, const Conv1x1WidePlan& p) {
  return conv1x1_wide_tiles(M, N, p) * p.splits * kCwTile * p.bn;
}

void launch_conv1x1_wide(const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t M, int K, int N,
                         const Conv1x1WidePlan& p, float* part, float* ws, unsigned* counters, hipStream_t s) {
  const dim3 grid(p.gx * (N / p.bn) * p.splits), block(kCwThreads);
#define RLA_CW_LAUNCH(B, SP)                                                                                      \
  hipLaunchKernelGGL((conv1x1_wide_kernel<B, SP>), grid, block, 0, s, x, w, y, M, K, N, p.tiles_per_blk, p.splits, \
                     part, ws, counters)
  if (p.bn == 256) {
    if (p.splits > 1)
      RLA_CW_LAUNCH(256, true);
    else
      RLA_CW_LAUNCH(256, false);
  } else {
    if (p.splits > 1)
      RLA_CW_LAUNCH(128, true);
    else
      RLA_CW_LAUNCH(128, false);
  }
#undef RLA_CW_LAUNCH
}

}  // namespace rla
