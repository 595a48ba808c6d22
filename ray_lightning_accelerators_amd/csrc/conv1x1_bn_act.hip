// 1x1 / stride-1 NHWC bf16 convolution forward with an EVAL-mode BatchNorm, the ReLU and the
// shortcut add in its epilogue (gfx950): the inference fusion of ResNet's conv1 -> bn1,
// conv3 -> bn3 (+ identity) and layer1.0.downsample.
//
//   out[m][n] = bf16(act(fma(acc[m][n], scale[n], shift[n]) + res[m][n]))
//   acc[m][n] = sum_k x[m][k] * w[n][k]          (fp32, never rounded to bf16, never written)
//   scale[n]  = gamma[n] / sqrt(var[n] + eps),   shift[n] = fma(-mean[n], scale[n], beta[n])
//
// Against the split route (a GEMM, four or five small torch ops for scale / shift, then
// bn_apply over the whole activation) this deletes one write and one read of every 1x1
// output, the coefficient launches, and one rounding per element.
//
// The GEMM is conv1x1.hip's: both operands K-contiguous rows, 256-thread workgroups = 2 pixel
// halves x 2 channel halves, a wave 64 pixels x 32 channels = 2 blocks of
// v_mfma_f32_32x32x16_bf16, the workgroup a 128-pixel x 64-channel tile; a K stage is 32
// channels, x [4 k units][128 rows] (+ w [4 k units][64 rows]) of 16 B, unit-major, by
// global_load_lds_dwordx4 (lds_dma.h) into a ring of 4 stages; a stage is retired by a counted
// vmcnt and one raw barrier; a workgroup walks `tiles_per_blk` consecutive pixel tiles of ONE
// channel column and the ring runs on across them; the gy channel columns of a pixel range
// run on one XCD (x comes from HBM once).  Rows past M read a clamped row and are not stored;
// stages past the end re-load the last one, so every iteration issues the same DMA count.
//   * K <= 128 (WRES): the column's whole weight block [K / 8 units][64 rows] (<= 16 KB) is
//     DMA'd once and stays in LDS; the ring carries x only (8 KB stages);
//   * larger K: x + w stream through the ring (12 KB stages).
//
// The epilogue is this kernel's own:
//   * coefficients in the prologue: the workgroup owns one channel column for all its tiles,
//     so threads 0 .. 63 compute its scale / shift from mean, var, gamma, beta and eps into a
//     512-byte LDS table ahead of the first DMA (the only compiler-visible loads of the
//     kernel), and every lane then keeps the 2 x 16 coefficients of its channels in registers;
//   * D of 32x32x16 gives a lane one pixel and channels 8 q + 4 h + e per accumulator 4 q + e;
//     one v_permlane32_swap per fp32 accumulator pair (q, q + 1) gives lane h the 8
//     consecutive channels 16 p + 8 h .. +8 of its pixel -- in fp32, ahead of the one rounding;
//   * the residual arrives by LDS-DMA, not through compiler-visible loads (which the compiler
//     waits for in order, draining the ring: conv1x1.hip BWD, docs/resnet50.md).  Each LANE
//     fetches exactly the 4 x 16 bytes it will consume -- pixel block j, channel group p, its
//     own (pixel, 8 channels) -- with 4 DMA instructions per wave into the wave's own 4 KB of
//     a 16 KB residual tile; the lane-linear DMA layout puts them at lane * 16 of each 1 KB
//     instruction block, so the epilogue reads them back with one conflict-free ds_read_b128
//     per 16-byte store.  Nobody but the issuing wave reads the block: no barrier guards it,
//     the wave's own lgkmcnt(0) after the last read releases it, and the NEXT tile's residual
//     is issued right there, in flight behind that tile's whole K loop.  The counted stage
//     waits include the residual DMA issued after the stage (a 3-bit history of which of the
//     last three iterations ended a tile), and the epilogue's own wait leaves only the stages
//     issued after the residual outstanding.
// LDS: 4 x 12 KB (or 4 x 8 + 16 KB resident weights) + 16 KB residual + the table = 64.5 KB,
// two workgroups per CU.  Every out element is written once, no atomics, and a tile's bits do
// not depend on the plan (each element's k order is fixed).
// Requires K % 32 == 0, N % 64 == 0, 16-byte aligned bases (binding checks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"
#include "lds_dma.h"

namespace rla {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBaThreads = 256;
constexpr int kBaTileM = 128;  // pixels per tile
constexpr int kBaTileN = 64;   // channels per workgroup column
constexpr int kBaStageK = 32;  // channels per K stage
constexpr int kBaStages = 4;   // ring depth
constexpr int kBaWResK = 128;  // largest K whose weight block stays resident
constexpr int kBaLdsBytes = 65536 + 2 * kBaTileN * 4;

enum { kEpiAffine = 0, kEpiRelu = 1, kEpiReluRes = 2 };

template <bool WRES, int EPI>
__global__ __launch_bounds__(kBaThreads, 2) void conv1x1_bn_act_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, const uint16_t* __restrict__ res,
    uint16_t* __restrict__ out, const float* __restrict__ mean, const float* __restrict__ var,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int M, int K, int N,
    int tiles_per_blk) {
  constexpr int NS = kBaStages, BN = kBaTileN;
  constexpr bool RES = EPI == kEpiReluRes;
  constexpr int kXBytes = 4 * kBaTileM * 16;  // x part of a stage: [4 k units][128 rows] x 16 B
  constexpr int kStageBytes = kXBytes + (WRES ? 0 : 4 * BN * 16);
  constexpr int kXInst = 2, kWInst = WRES ? 0 : 1;  // DMA instructions per wave per stage
  constexpr int kDma = kXInst + kWInst;
  constexpr int kWResBytes = WRES ? (kBaWResK / 8) * BN * 16 : 0;
  constexpr int kResInst = RES ? 4 : 0;  // residual DMA instructions per wave per tile
  constexpr int kResBytes = RES ? kBaTileM * BN * 2 : 0;
  static_assert(NS * kStageBytes + kWResBytes + kResBytes + 2 * BN * 4 <= kBaLdsBytes, "LDS plan");
  static_assert(2 * kBaLdsBytes <= 160 * 1024, "LDS budget (two workgroups per CU)");
  static_assert(NS == 4, "the wait counts are written out for a ring of 4");
  // one array, so that it starts at LDS address 0 and every DMA target lies below 64 KB;
  // the coefficient table [scale | shift][64] sits behind the DMA regions
  constexpr int kTabOff = NS * kStageBytes + kWResBytes + kResBytes;
  __shared__ __attribute__((aligned(16))) uint8_t ring[kTabOff + 2 * BN * 4];
  float(*tab)[BN] = reinterpret_cast<float(*)[BN]>(ring + kTabOff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1, r = lane & 31, h = lane >> 5;
  // XCD-aware (x, y): hardware block b runs on XCD b % 8; the gy channel columns of pixel
  // range x all sit on XCD x % 8 (the grid's range count is a multiple of 8)
  const int gy = N / BN;
  const int xcd = (int)(blockIdx.x % 8u), slot = (int)(blockIdx.x / 8u);
  const int bx = xcd + 8 * (slot / gy), by = slot % gy;
  const int mt = (M + kBaTileM - 1) / kBaTileM;
  const int t0 = bx * tiles_per_blk;
  const int ntiles = mt - t0 < tiles_per_blk ? mt - t0 : tiles_per_blk;
  if (ntiles <= 0) return;  // padding range of the XCD deal: nothing to write
  const int nb = by * BN;   // workgroup's first channel
  const int cw = wn * 32;   // wave's first channel within the column

  // the column's coefficients, ahead of every DMA: the counted waits below see DMA only
  if (tid < BN) {
    const float sc = gamma[nb + tid] / sqrtf(var[nb + tid] + eps);
    tab[0][tid] = sc;
    tab[1][tid] = __builtin_fmaf(-mean[nb + tid], sc, beta[nb + tid]);
  }
  __syncthreads();
  float sc[2][8], sh[2][8];  // channels cw + 16 p + 8 h .. +8: what the lane holds after the swap
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&tab[0][cw + 16 * p + 8 * h + 4 * q]);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&tab[1][cw + 16 * p + 8 * h + 4 * q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sc[p][4 * q + e] = a[e];
        sh[p][4 * q + e] = b[e];
      }
    }

  const int nch = K / kBaStageK;
  const int nst = ntiles * nch;
  const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)ring;
  const uint32_t wres0 = ring0 + NS * kStageBytes;
  constexpr int kResOff = NS * kStageBytes + kWResBytes;

  // DMA of stage st into ring buffer st % NS: wave-instruction g of the x part covers k unit
  // g / 2, rows 64 (g & 1) .. +64; the wave's one instruction of the w part k unit `wave`
  int ist = 0, iti = 0, ic = 0;  // the next stage to issue, its tile and chunk (clamped at the end)
  auto issue = [&]() {
    const int k = ic * kBaStageK;
    const uint32_t buf = ring0 + (uint32_t)(ist % NS) * kStageBytes;
#pragma unroll
    for (int u = 0; u < kXInst; ++u) {
      const int g = wave * kXInst + u;
      int m = (t0 + iti) * kBaTileM + (g & 1) * 64 + lane;
      m = m < M ? m : M - 1;
      c1_dma16(x + (int64_t)m * K + k + 8 * (g >> 1), __builtin_amdgcn_readfirstlane(buf + g * 1024));
    }
    if constexpr (!WRES)
      c1_dma16(w + (int64_t)(nb + lane) * K + k + 8 * wave,
               __builtin_amdgcn_readfirstlane(buf + kXBytes + wave * 1024));
    ++ist;
    if (ist < nst && ++ic == nch) ic = 0, ++iti;
  };
  // residual of tile ti: instruction (j, p) = the lane's own pixel 32 j + r, channels
  // cw + 16 p + 8 h .. +8, landing at lane * 16 of block 2 j + p of the wave's 4 KB
  auto issue_res = [&](int ti) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int m = (t0 + ti) * kBaTileM + wm * 64 + 32 * j + r;
      m = m < M ? m : M - 1;
#pragma unroll
      for (int p = 0; p < 2; ++p)
        c1_dma16(res + (int64_t)m * N + nb + cw + 16 * p + 8 * h,
                 __builtin_amdgcn_readfirstlane(ring0 + kResOff + wave * 4096 + (2 * j + p) * 1024));
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) acc[j] = f32x16{};

  // lane l of v_mfma_f32_32x32x16_bf16: row l & 31, k = 8 (l >> 5) .. +8 of both operands
  auto compute = [&](int st, int c) {
    const uint8_t* buf = ring + (st % NS) * kStageBytes;
    const uint8_t* wb = WRES ? ring + NS * kStageBytes + c * 4 * BN * 16 : buf + kXBytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ku = 2 * ks + h;
      const bf16x8 fa = *reinterpret_cast<const bf16x8*>(wb + (ku * BN + cw + r) * 16);
      bf16x8 fb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[j] = *reinterpret_cast<const bf16x8*>(buf + (ku * kBaTileM + wm * 64 + 32 * j + r) * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[j], acc[j], 0, 0, 0);
    }
  };

  auto epilogue = [&](int ti) {
    const int m0 = (t0 + ti) * kBaTileM + wm * 64 + r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + 32 * j;
      const bool ok = m < M;  // lanes l and l ^ 32 share the pixel: the swap stays in-pixel
      uint16_t* yo = out + (int64_t)(ok ? m : 0) * N + nb + cw + 8 * h;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // (the elements by value: a bit cast of the vector-element lvalue itself reads element 0)
          const float lo = acc[j][8 * p + e], hi = acc[j][8 * p + 4 + e];
          const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
          v[e] = __uint_as_float(s[0]);
          v[4 + e] = __uint_as_float(s[1]);
        }
        bf16x8 rr;
        if constexpr (RES)
          rr = *reinterpret_cast<const bf16x8*>(ring + kResOff + wave * 4096 + (2 * j + p) * 1024 + lane * 16);
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float a = __builtin_fmaf(v[k], sc[p][k], sh[p][k]);
          if constexpr (RES) a += (float)rr[k];
          if constexpr (EPI != kEpiAffine) a = a > 0.f ? a : 0.f;
          o[k] = (__bf16)a;
        }
        if (ok) *reinterpret_cast<bf16x8*>(yo + 16 * p) = o;
      }
      acc[j] = f32x16{};
    }
  };

  if constexpr (WRES) {  // the weight block, ahead of stage 0 (retired by stage 0's counted wait)
    for (int g = wave; g < K / 8; g += 4)
      c1_dma16(w + (int64_t)(nb + lane) * K + 8 * g, __builtin_amdgcn_readfirstlane(wres0 + g * 1024));
  }
  if constexpr (RES) issue_res(0);
#pragma unroll
  for (int d = 0; d < NS - 1; ++d) issue();

#define RLA_BA_WAIT(N) asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory")
  // hist bit b: iteration st - 1 - b ended a tile, i.e. issued a residual tile AFTER stage
  // st's DMA (stage st went out at the top of iteration st - 3, or in the prologue)
  uint32_t hist = 0;
  int ti = 0, c = 0;
  for (int st = 0; st < nst; ++st) {
    // stage st landed: the DMA issued after it (NS - 2 stages and the residual tiles of
    // `hist`) may still fly; then every wave's part is in and every wave has finished
    // reading buffer st - 1, which the next issue overwrites
    if constexpr (RES) {
      switch (__builtin_popcount(hist & 7u)) {
        case 0: RLA_BA_WAIT((NS - 2) * kDma); break;
        case 1: RLA_BA_WAIT((NS - 2) * kDma + kResInst); break;
        case 2: RLA_BA_WAIT((NS - 2) * kDma + 2 * kResInst); break;
        default: RLA_BA_WAIT((NS - 2) * kDma + 3 * kResInst); break;
      }
    } else {
      RLA_BA_WAIT((NS - 2) * kDma);
    }
    issue();
    compute(st, c);
    const bool last = c == nch - 1;
    if (last) {
      if constexpr (RES) {
        // this tile's residual went out before the stages of the tile's own nch iterations
        // (tile 0: before the prologue's too): at most that many, and never more than the
        // NS - 1 stages that can be in flight, were issued after it
        if (nch == 1)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kDma) : "memory");
        else if (nch == 2)
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * kDma) : "memory");
        else
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * kDma) : "memory");
      }
      epilogue(ti);
      if constexpr (RES) {
        if (ti + 1 < ntiles) {
          // the wave's own reads of its residual block are done: the next tile's may land
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          issue_res(ti + 1);
        }
      }
      ++ti, c = 0;
    } else {
      ++c;
    }
    hist = (hist << 1) | (last ? 1u : 0u);
  }
#undef RLA_BA_WAIT
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may outlive the workgroup's LDS
}

}  // namespace

Conv1x1BnActGeom conv1x1_bn_act_geom(int64_t M, int64_t K, int64_t N) {
  Conv1x1BnActGeom g{};
  const int64_t lim = int64_t(1) << 31;
  // 32-bit row indexing with room for a short last tile's row numbers past M
  if (M <= 0 || K <= 0 || N <= 0 || M >= lim - 2 * kBaTileM || K > 8192 || N > 8192) return g;
  const int64_t mt = (M + kBaTileM - 1) / kBaTileM, gy = N / kBaTileN;
  if (gy == 0) return g;
  // ~2 resident workgroups per CU over the whole grid; pixel ranges a multiple of 8 (XCD deal,
  // the ranges past the last tile exit at once).  No floor of 8 ranges: a plan pinned to a
  // few CUs then walks several tiles per workgroup even at a few hundred rows (tests)
  int64_t want = 2 * (int64_t)plan_cus() / gy;
  if (want < 1) want = 1;
  if (want > mt) want = mt;
  const int64_t tpb = (mt + want - 1) / want;
  const int64_t gx = ((mt + tpb - 1) / tpb + 7) / 8 * 8;
  if (gx * gy >= lim) return g;
  g.M = (int)M, g.K = (int)K, g.N = (int)N;
  g.rows = (int)mt, g.cols = (int)gy, g.tiles_per_blk = (int)tpb, g.gx = (int)gx, g.grid = (int)(gx * gy);
  g.wres = K <= kBaWResK;
  return g;
}

bool conv1x1_bn_act_ok(const Conv1x1BnActGeom& g) {
  return g.M > 0 && g.K >= kBaStageK && g.K % kBaStageK == 0 && g.N % kBaTileN == 0 && g.cols > 0;
}

int conv1x1_bn_act_tile_m() { return kBaTileM; }
int conv1x1_bn_act_tile_n() { return kBaTileN; }
int conv1x1_bn_act_stages() { return kBaStages; }
int conv1x1_bn_act_lds_bytes() { return kBaLdsBytes; }

bool launch_conv1x1_bn_act(const uint16_t* x, const uint16_t* w, const uint16_t* res, uint16_t* out,
                           const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                           bool relu, const Conv1x1BnActGeom& g, hipStream_t stream) {
  if (!conv1x1_bn_act_ok(g) || (res && !relu)) return false;
  const dim3 grid(g.grid), block(kBaThreads);
#define RLA_BA_LAUNCH(R, E)                                                                                      \
  hipLaunchKernelGGL((conv1x1_bn_act_kernel<R, E>), grid, block, 0, stream, x, w, res, out, mean, var, gamma, beta, \
                     eps, g.M, g.K, g.N, g.tiles_per_blk)
  const int epi = res ? kEpiReluRes : (relu ? kEpiRelu : kEpiAffine);
  if (g.wres) {
    if (epi == kEpiReluRes)
      RLA_BA_LAUNCH(true, kEpiReluRes);
    else if (epi == kEpiRelu)
      RLA_BA_LAUNCH(true, kEpiRelu);
    else
      RLA_BA_LAUNCH(true, kEpiAffine);
  } else {
    if (epi == kEpiReluRes)
      RLA_BA_LAUNCH(false, kEpiReluRes);
    else if (epi == kEpiRelu)
      RLA_BA_LAUNCH(false, kEpiRelu);
    else
      RLA_BA_LAUNCH(false, kEpiAffine);
  }
#undef RLA_BA_LAUNCH
  return true;
}

}  // namespace rla
