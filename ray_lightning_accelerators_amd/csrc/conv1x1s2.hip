// 1x1 / stride-2 / pad-0 NHWC bf16 convolution forward (gfx950), plain and with the
// following BatchNorm's batch statistics in its epilogue: ResNet-50's downsample shortcuts.
//
//   y[n][ho][wo][c] = bf16(sum_k x[n][2 ho][2 wo][k] * w[c][k]),  OH = (H - 1) / 2 + 1, OW likewise
//   part[b][0][c] = sum over the 128 output pixels of row tile b of bf16(y),  part[b][1][c] = of its square
//
// (the ROUNDED values are summed, conv1x1.hip's and conv3x3s2.hip's convention, so `part` is
// what BatchNorm's own pass over y would have produced).  A GEMM over the M = N OH OW output
// pixels whose A rows are GATHERED: output row m = (n OH + ho) OW + wo reads the Cin
// contiguous bf16 of input row (n H + 2 ho) W + 2 wo; odd rows and columns of x are never read.
//
// Work split -- output-tile ownership, no split-K, no atomics, every y element written once:
//   * a 256-thread workgroup (4 waves = 2 pixel halves x 2 channel halves) owns 128 output
//     pixels x 128 output channels; a wave 64 x 64 = 2 x 2 blocks of
//     v_mfma_f32_32x32x16_bf16 (64 accumulators).  32x32x16 and not 16x16x32: a fragment read
//     feeds 32 x 32 outputs, half the LDS reads per flop of the 16 x 16 form, and its D layout
//     (lane = pixel, 4 consecutive channels per accumulator group) is the one the tree's
//     16-byte-store epilogue is written for;
//   * tiles at batch 128 (256 CUs, two workgroups resident per CU by LDS: 64 / 65 KB each):
//       56x56 256 -> 512:   784 row tiles x  4 = 3136 tiles (6.1 rounds of 512)
//       28x28 512 -> 1024:  196 row tiles x  8 = 1568 tiles (3.1 rounds)
//       14x14 1024 -> 2048:  49 row tiles x 16 =  784 tiles (1.5 rounds; 56 row slots after
//                                                             the padding to a multiple of 8)
//   * the row map is computed ONCE per tile: a lane stages the same two A rows (64 u + lane,
//     u = 0, 1) in every K stage, so it keeps two gathered row pointers and only adds the
//     stage's channel offset.  Rows past M in a short last tile read row M - 1 (in range,
//     never stored, excluded from the sums);
//   * a K stage is 32 channels: x [4 k units][128 rows] and w [4 k units][128 rows] of 16 B,
//     unit-major (fragment reads are contiguous 512-B ds_read_b128 runs), both by per-lane
//     address LDS-DMA (lds_dma.h) into a ring of 4 stages of 16 KB.  A stage is retired by a
//     counted vmcnt and one raw barrier; the tail counts down (8, 4, 0 outstanding) instead of
//     re-loading a stage, so no byte is fetched twice (at Cin = 256 three re-loads would be
//     37 % more L2 traffic).  The loop holds no other load, and the epilogue's stores come
//     after the last wait;
//   * row tile bx's channel columns are dealt to one XCD (hardware block b runs on XCD
//     b % 8), next to each other in time: the gathered rows are fetched into that L2 once.
// Epilogue (conv1x1_wide.hip's register path): round to bf16, add the rounded values into the
// lane's per-channel sums (statistics instance), one v_permlane32_swap per dword pair widens
// the stores to 16 bytes per lane; then the lanes' sums go through the (now idle) ring and
// thread (statistic, channel) adds the tile's 64 pixel slots in slot order: fixed order, no
// float atomics, two runs agree bitwise.  (A butterfly over the pixel lanes, the first form
// of this reduction, cost 34 us of the 56x56 layer's 97: profiles/r24_conv1x1s2.)
// Requires Cin % 64 == 0, Cout % 128 == 0, 16-byte aligned bases, N H W < 2^31 (binding checks).
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

constexpr int kS2Threads = 256;
constexpr int kS2TileM = 128;  // output pixels per tile
constexpr int kS2TileN = 128;  // output channels per tile
constexpr int kS2StageK = 32;  // channels per K stage
constexpr int kS2Stages = 4;   // ring depth

template <bool ST>
__global__ __launch_bounds__(kS2Threads) void conv1x1s2_kernel(const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ w,
                                                               uint16_t* __restrict__ y, int M, int K, int N, int H,
                                                               int W, int OH, int OW, int mt,
                                                               float* __restrict__ part) {
  constexpr int NS = kS2Stages;
  constexpr int kXBytes = 4 * kS2TileM * 16;  // x part of a stage: [4 k units][128 rows] x 16 B
  constexpr int kStageBytes = kXBytes + 4 * kS2TileN * 16;
  constexpr int kDma = 4;  // DMA instructions per wave per stage: 2 of x, 2 of w
  // the statistics instance reuses the ring for its reduction: 2 x 32 channel groups of
  // [64 pixel slots][4 channels] floats, each padded by 4 floats
  constexpr int kRedGroup = 64 * 4 + 4;
  constexpr int kRedBytes = ST ? 2 * 32 * kRedGroup * 4 : 0;
  constexpr int kLdsBytes = NS * kStageBytes > kRedBytes ? NS * kStageBytes : kRedBytes;
  static_assert(2 * kLdsBytes <= 160 * 1024, "LDS budget (two workgroups per CU)");
  static_assert(NS == 4, "the tail's wait counts are written out for a ring of 4");
  __shared__ __attribute__((aligned(16))) uint8_t ring[kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1, r = lane & 31, h = lane >> 5;
  // XCD-aware deal: the gy channel columns of row tile bx all sit on XCD bx % 8 (the grid's
  // row count is a multiple of 8); only locality depends on it
  const int gy = N / kS2TileN;
  const int xcd = (int)(blockIdx.x % 8u), slot = (int)(blockIdx.x / 8u);
  const int bx = xcd + 8 * (slot / gy), by = slot % gy;
  if (bx >= mt) return;  // padding row slot: part has mt rows, nothing to write
  const int nb = by * kS2TileN;
  const int nst = K / kS2StageK;
  const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)ring;

  // the row map, once per tile: wave-instruction u of the x part covers k unit `wave`, rows
  // 64 u .. +64; of the w part the same unit, channels nb + 64 u .. +64
  const uint16_t* xsrc[2];
  const uint16_t* wsrc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    int m = bx * kS2TileM + 64 * u + lane;
    m = m < M ? m : M - 1;
    const int n = m / (OH * OW), rem = m - n * (OH * OW);
    const int ho = rem / OW, wo = rem - ho * OW;
    const int64_t row = ((int64_t)n * H + 2 * ho) * W + 2 * wo;
    xsrc[u] = x + row * K + 8 * wave;
    wsrc[u] = w + (int64_t)(nb + 64 * u + lane) * K + 8 * wave;
  }

  auto issue = [&](int st) {
    const uint32_t buf = ring0 + (uint32_t)(st % NS) * kStageBytes + (uint32_t)wave * 2048;
    const int k = st * kS2StageK;
#pragma unroll
    for (int u = 0; u < 2; ++u) c1_dma16(xsrc[u] + k, __builtin_amdgcn_readfirstlane(buf + u * 1024));
#pragma unroll
    for (int u = 0; u < 2; ++u) c1_dma16(wsrc[u] + k, __builtin_amdgcn_readfirstlane(buf + kXBytes + u * 1024));
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[t][j] = f32x16{};

  // lane l of v_mfma_f32_32x32x16_bf16: row l & 31, k = 8 (l >> 5) .. +8 of both operands
  auto compute = [&](int st) {
    const uint8_t* buf = ring + (st % NS) * kStageBytes;
    const uint8_t* wb = buf + kXBytes;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ku = 2 * s + h;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
        fa[t] = *reinterpret_cast<const bf16x8*>(wb + (ku * kS2TileN + wn * 64 + 32 * t + r) * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(buf + (ku * kS2TileM + wm * 64 + 32 * j + r) * 16);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[t], fb[j], acc[t][j], 0, 0, 0);
    }
  };

#pragma unroll
  for (int d = 0; d < NS - 1; ++d)
    if (d < nst) issue(d);
  for (int st = 0; st < nst; ++st) {
    // stage st landed: only the DMA of the stages issued after it (at most NS - 2, fewer in
    // the tail) may still fly; then every wave's part is in and every wave has finished
    // reading buffer st - 1, which the next issue overwrites
    const int after = nst - 1 - st;
    if (after >= 2)
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(2 * kDma) : "memory");
    else if (after == 1)
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(kDma) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (st + NS - 1 < nst) issue(st + NS - 1);
    compute(st);
  }
  // every DMA was waited for above (the last iteration's vmcnt(0)): none outlives the LDS

  // D[c][m]: lane -> pixel r of block j; accumulator 4q + e -> channel 8q + 4h + e.
  // One v_permlane32_swap per dword of each channel-group pair (q, q + 1) gives lane h
  // channels 16p + 8h .. +8: one 16-byte store where the MFMA layout gives two of 8
  float ssum[2][16], ssq[2][16];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) ssum[t][e] = ssq[t][e] = 0.f;
  const int cw = nb + wn * 64;  // wave's first channel
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = bx * kS2TileM + wm * 64 + 32 * j + r;
    const bool ok = m < M;  // lanes l and l ^ 32 share the pixel: the swap stays in-pixel
    uint16_t* yo = y + (int64_t)(ok ? m : 0) * N + cw + 8 * h;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      uint32_t v[4][2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (__bf16)acc[t][j][4 * q + e];
        if (ST && ok) {
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
  }

  if constexpr (ST) {
    // per-channel totals through the ring, which nobody reads any more: every lane leaves its
    // 2 x 32 sums as 16-byte groups of 4 consecutive channels, red[stat][channel group]
    // [64 pixel slots][4] (a group's stride padded by 4 floats: the 16 groups x 4 channels a
    // wave reads below fall into 64 different banks); then thread (stat, channel) adds its 64
    // slots in slot order -- a fixed order, where a butterfly over the pixel lanes costs
    // 640 cross-lane operations per lane
    float* red = reinterpret_cast<float*>(ring);
    __syncthreads();  // every wave has finished reading the last stage
    const int slot = wm * 32 + r;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cg = wn * 16 + 8 * t + 2 * q + h;  // channels 4 cg .. +4 of the tile
        const f32x4 a = {ssum[t][4 * q], ssum[t][4 * q + 1], ssum[t][4 * q + 2], ssum[t][4 * q + 3]};
        const f32x4 b = {ssq[t][4 * q], ssq[t][4 * q + 1], ssq[t][4 * q + 2], ssq[t][4 * q + 3]};
        *reinterpret_cast<f32x4*>(red + cg * kRedGroup + slot * 4) = a;
        *reinterpret_cast<f32x4*>(red + (32 + cg) * kRedGroup + slot * 4) = b;
      }
    __syncthreads();
    const int stat = tid >> 7, c = tid & 127;
    const float* src = red + (stat * 32 + (c >> 2)) * kRedGroup + (c & 3);
    float tot = 0.f;
#pragma unroll 16
    for (int s = 0; s < 64; ++s) tot += src[4 * s];
    part[(int64_t)bx * 2 * N + (int64_t)stat * N + nb + c] = tot;
  }
}

}  // namespace

Conv1x1S2Geom conv1x1s2_geom(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
  Conv1x1S2Geom g{};
  const int64_t lim = int64_t(1) << 31;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || N >= lim || H >= lim || W >= lim || Cin >= lim / 2 ||
      Cout >= lim / 2)
    return g;
  // 32-bit row indexing: input rows N H W (each factor below 2^31, so no product overflows),
  // with room for a short last tile's row numbers past M
  if (N * H >= lim || N * H * W >= lim - 2 * kS2TileM) return g;
  const int64_t oh = (H - 1) / 2 + 1, ow = (W - 1) / 2 + 1, m = N * oh * ow;
  const int64_t mt = (m + kS2TileM - 1) / kS2TileM, gx = (mt + 7) / 8 * 8, gy = Cout / kS2TileN;
  if (gx * (gy > 0 ? gy : 1) >= lim) return g;
  g.N = (int)N, g.H = (int)H, g.W = (int)W, g.Cin = (int)Cin, g.Cout = (int)Cout;
  g.OH = (int)oh, g.OW = (int)ow, g.M = (int)m;
  g.rows = (int)mt, g.cols = (int)gy, g.grid = (int)(gx * gy);
  return g;
}

bool conv1x1s2_ok(const Conv1x1S2Geom& g) {
  return g.N > 0 && g.Cin >= 64 && g.Cin % 64 == 0 && g.Cout % kS2TileN == 0 && g.cols > 0;
}

int conv1x1s2_tile_m() { return kS2TileM; }
int conv1x1s2_tile_n() { return kS2TileN; }
int conv1x1s2_stage_k() { return kS2StageK; }
int conv1x1s2_stages() { return kS2Stages; }

bool launch_conv1x1s2(const uint16_t* x, const uint16_t* w, uint16_t* y, const Conv1x1S2Geom& g, hipStream_t stream,
                      float* part) {
  if (!conv1x1s2_ok(g)) return false;
  const dim3 grid(g.grid), block(kS2Threads);
  if (part)
    hipLaunchKernelGGL(conv1x1s2_kernel<true>, grid, block, 0, stream, x, w, y, g.M, g.Cin, g.Cout, g.H, g.W, g.OH,
                       g.OW, g.rows, part);
  else
    hipLaunchKernelGGL(conv1x1s2_kernel<false>, grid, block, 0, stream, x, w, y, g.M, g.Cin, g.Cout, g.H, g.W, g.OH,
                       g.OW, g.rows, part);
  return true;
}

}  // namespace rla
