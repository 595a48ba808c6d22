// Input gradient of a 1x1 / stride-1 NHWC bf16 convolution with 128 < K <= 512 output
// channels, fused with the PREVIOUS BatchNorm's backward partial pass (gfx950).
//
//   da[m][n]  = bf16(sum_k dy1[m][k] * w[k][n])        (fp32 MFMA sum; w is the FORWARD weight
//                                                       [Cout = K][Cin = N], read as stored)
//   d[m][n]   = bf16(yb[m][n] > 0 ? float(da) + float(dy2[m][n]) : 0)
//   part[t][0][n] = sum over the valid pixels of 128-pixel tile t of float(d)
//   part[t][1][n] = the same of float(d) * float(xb[m][n])
//
// These are the semantics of conv1x1.hip's BWD epilogue (K <= 128); that kernel keeps its
// whole weight block resident beside a ring that streams dy1, which stops fitting at K = 256.
// Here the roles are swapped -- the layer is bound by the four [M, N] epilogue streams
// (dy2, yb, xb in, d out), not by MFMA, so the design keeps those streams busy:
//   * pixel-stationary: a 256-thread workgroup (2 channel halves x 2 pixel halves of waves)
//     walks a contiguous range of UNITS = (128-pixel tile, group of up to four 64-channel
//     column blocks), tile-major, so consecutive units share their pixel tile.  The dy1 tile
//     (128 x K bf16: 64 KB at K = 256, 128 KB at K = 512) is brought into LDS by LDS-DMA once
//     per tile, 16-byte-unit-major ([k unit][row]: conv1x1.hip's conflict-free fragment
//     layout), and is re-loaded only when the next unit is on another tile;
//   * only the weights stream: a stage is 32 k rows x 64 channels of w (4 KB, one DMA
//     instruction per wave), a ring of NS stages retired by COUNTED vmcnt waits and one raw
//     barrier each (conv1x1.hip's scheme; the DMA is inline asm the compiler's wait
//     bookkeeping does not see).  The ring runs on across column blocks and units.  The
//     weight is read in its stored layout: a stage is [32 k][64 n] rows of 128 B whose
//     16-byte pieces are XOR-swizzled by k & 7 by the DMA's source addresses, and the A
//     fragments come from transposed LDS reads (ds_read_b64_tr_b16, conv_wgrad.hip's lane
//     roles), so no transposed copy of the weight is made per step;
//   * the three 16-byte epilogue operand streams of column block c + 1 are loaded at block
//     c's first stage into the other of two fixed register sets (the block loop is unrolled
//     by two); the counted stage waits that follow include those 12 loads, so the
//     compiler's in-order wait for them never drains the ring (round-6 BWD lesson);
//   * v_mfma_f32_32x32x16_bf16, D[n][m]: a lane holds one pixel and 4 consecutive channels
//     per 4 accumulators; one v_permlane32_swap per dword pair widens the d stores to 16 B;
//   * statistics: per-lane fp32 sums of the block's two pixel sub-blocks, a reduce-scatter
//     butterfly over the 32 pixel lanes (31 exchanges for the 32 values, where a plain
//     butterfly takes 160), then the two pixel-half waves in a fixed order through LDS.
//     One partial row per PIXEL TILE: every (tile, column block) owns its 64 floats of both
//     rows and writes them exactly once, so nothing is carried, zero-filled or atomic, and
//     two calls are bitwise equal.  rows = ceil(M / 128) whatever the grid;
//   * grid: min(units, resident workgroups over plan_cus()) rounded up to 8, workgroup b
//     taking the (b % 8)-th eighth of the unit ranges, so the units of a pixel tile run on
//     one XCD (dy1 from HBM once, the 0.5 / 2 MB weight from that XCD's L2).
// Departures from the recommended design: statistics are one row per tile rather than
// carried across a workgroup's units (nothing to carry: a unit's channels are its own), and
// a tile change drains the ring once (s_waitcnt vmcnt(0)) before the new dy1 tile is read --
// the ring's stages stay valid and refill behind the next block.
// Two instances: K <= 256 with NS = 3 stages beside a 64 KB tile image (77 KB of LDS, within
// 256 registers: two workgroups per CU, one in its epilogue while the other multiplies) and
// K <= 512 with NS = 7 beside 128 KB (157 KB: one workgroup per CU).
// Rows past M read a clamped row, are never stored and never summed; ring stages past the
// end re-load the last one.
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
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kBwThreads = 256;
constexpr int kBwTileM = 128;         // pixels per tile = per partial row
constexpr int kBwGroupBlocks = 4;     // 64-channel column blocks per unit
constexpr int kBwStageBytes = 32 * 64 * 2;
constexpr int kBwSmallK = 256;        // the small instance: tile image 128 x 256, 3 ring stages
constexpr int kBwSmallStages = 3;
constexpr int kBwMaxK = 512;          // the large one: 128 x 512, 7 stages
constexpr int kBwStages = 7;
constexpr int kBwPreLoads = 12;       // epilogue operand loads per lane and column block

__device__ __forceinline__ bf16x4 bw_tr4(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(p));
}

__device__ __forceinline__ bf16x8 bw_cat8(bf16x4 lo, bf16x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// stage `st` landed (EXTRA younger operand loads may still fly besides the NS - 2 younger
// stages), every wave's LDS reads of the previous stage are done
template <int CNT>
__device__ __forceinline__ void bw_wait() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(CNT) : "memory");
}

template <int NS, int KMAX>
__global__ __launch_bounds__(kBwThreads, KMAX <= 256 ? 2 : 1) void conv1x1_bn_bwd_wide_kernel(
    const uint16_t* __restrict__ dy1, const uint16_t* __restrict__ w, uint16_t* __restrict__ d, int64_t M, int K, int N,
    int groups, int64_t units, const uint16_t* __restrict__ dy2, const uint16_t* __restrict__ yb,
    const uint16_t* __restrict__ xb, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[KMAX * 256];  // [K / 8 units][128 rows] x 16 B
  __shared__ __attribute__((aligned(16))) uint8_t ring[NS * kBwStageBytes];
  __shared__ float red[2][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1, r = lane & 31, h = lane >> 5;
  // XCD deal: hardware block b runs on XCD b % 8 and takes logical range (b % 8) G / 8 + b / 8
  const int G = (int)gridDim.x;
  const int lw = (int)(blockIdx.x % 8u) * (G / 8) + (int)(blockIdx.x / 8u);
  const int64_t u0 = units * lw / G, u1 = units * (lw + 1) / G;
  if (u0 >= u1) return;
  const int nch = K >> 5, ncol = N >> 6;
  const uint32_t tile0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)tile;
  const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)ring;

  auto unit_ncb = [&](int g) { return ncol - kBwGroupBlocks * g < kBwGroupBlocks ? ncol - kBwGroupBlocks * g : kBwGroupBlocks; };

  // dy1 tile t: wave-instruction g covers k unit g / 2, rows 64 (g & 1) .. +64
  auto load_tile = [&](int t) {
    for (int g = wave; g < K / 4; g += 4) {
      int64_t m = (int64_t)t * kBwTileM + (g & 1) * 64 + lane;
      m = m < M ? m : M - 1;
      c1_dma16(dy1 + m * K + 8 * (g >> 1), __builtin_amdgcn_readfirstlane(tile0 + g * 1024));
    }
  };

  // weight stages, in stream order over (unit, column block, 32-row k chunk): this wave's
  // instruction covers stage rows 8 wave .. +8 (lane >> 3), the row's eight 16-byte pieces
  // stored at slot piece ^ (row & 7)
  const uint16_t* wlane = w + (int64_t)(8 * wave + (lane >> 3)) * N + 8 * ((lane & 7) ^ (lane >> 3));
  int64_t iu = u0;
  int ig = (int)(u0 % groups), ic = 0, ik = 0, incb = unit_ncb(ig), ist = 0;
  auto issue = [&]() {
    c1_dma16(wlane + (int64_t)ik * 32 * N + (kBwGroupBlocks * ig + ic) * 64,
             __builtin_amdgcn_readfirstlane(ring0 + (uint32_t)(ist % NS) * kBwStageBytes + wave * 1024));
    ++ist;
    if (ik + 1 < nch) {
      ++ik;
    } else if (ic + 1 < incb) {
      ik = 0, ++ic;
    } else if (iu + 1 < u1) {
      ik = 0, ic = 0, ++iu;
      ig = ig + 1 < groups ? ig + 1 : 0;
      incb = unit_ncb(ig);
    }  // else: the stream's last stage again
  };

  // transposed-read lane roles (conv_wgrad.hip): 16-lane group gq, lane 4q + p addresses k row
  // q, channels 4p .. 4p + 3; the two reads of a fragment are k rows rwo and rwo + 4
  const int gq = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  const int wch = wn * 32 + 16 * (gq & 1) + 4 * tp;  // channel inside the 64-channel block
  const int rwo = 8 * (gq >> 1) + tq;                // k row inside a 16-row step
  const int aoff0 = rwo * 128 + (((wch >> 3) ^ tq) << 4) + (wch & 7) * 2;
  const int aoff1 = (rwo + 4) * 128 + (((wch >> 3) ^ (tq + 4)) << 4) + (wch & 7) * 2;
  const int boff = (wm * 64 + r) * 16;

  f32x16 acc[2] = {f32x16{}, f32x16{}};
  auto compute = [&](int st, int kc) {
    const uint8_t* buf = ring + (st % NS) * kBwStageBytes;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 fa = bw_cat8(bw_tr4(buf + ks * 2048 + aoff0), bw_tr4(buf + ks * 2048 + aoff1));
      const uint8_t* tb = tile + ((kc * 4 + 2 * ks + h) * 128) * 16 + boff;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, *reinterpret_cast<const bf16x8*>(tb + 32 * j * 16), acc[j],
                                                         0, 0, 0);
    }
  };

  // dy2 / yb / xb of a block's [2 pixel sub-blocks][2 channel halves] 16-byte chunks
  typedef u32x4 PreSet[3][2][2];
  auto prefetch = [&](PreSet& pre, int t, int n0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      int64_t m = (int64_t)t * kBwTileM + wm * 64 + 32 * j + r;
      m = m < M ? m : M - 1;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int64_t off = m * N + n0 + wn * 32 + 16 * p + 8 * h;
        pre[0][j][p] = *reinterpret_cast<const u32x4*>(dy2 + off);
        pre[1][j][p] = *reinterpret_cast<const u32x4*>(yb + off);
        pre[2][j][p] = *reinterpret_cast<const u32x4*>(xb + off);
      }
    }
  };

  // D[n][m]: lane -> pixel r of sub-block j; accumulator 4q + e -> channel 8q + 4h + e.  One
  // v_permlane32_swap per dword of each channel-group pair (q, q + 1) gives lane h channels
  // 16p + 8h .. +8: one 16-byte store.  sv[8p + k] / sv[16 + 8p + k]: the lane's sums of d
  // and d * xb for channel 16p + 8h + k of the wave's 32
  float sv[32];
  auto epilogue = [&](int t, int n0, const PreSet& pre) {
    const int64_t m0 = (int64_t)t * kBwTileM + wm * 64 + r;
#pragma unroll
    for (int e = 0; e < 32; ++e) sv[e] = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t m = m0 + 32 * j;
      const bool ok = m < M;  // lanes l and l ^ 32 share the pixel: the swap stays in-pixel
      uint16_t* dout = d + (ok ? m : 0) * N + n0 + wn * 32 + 8 * h;
      uint32_t v[4][2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (__bf16)acc[j][4 * q + e];
        const u32x2 pk = __builtin_bit_cast(u32x2, b);
        v[q][0] = pk[0];
        v[q][1] = pk[1];
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const auto s0 = __builtin_amdgcn_permlane32_swap(v[2 * p][0], v[2 * p + 1][0], false, false);
        const auto s1 = __builtin_amdgcn_permlane32_swap(v[2 * p][1], v[2 * p + 1][1], false, false);
        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
        const bf16x8 da = __builtin_bit_cast(bf16x8, o);
        const bf16x8 g2 = __builtin_bit_cast(bf16x8, pre[0][j][p]);
        const bf16x8 ym = __builtin_bit_cast(bf16x8, pre[1][j][p]);
        const bf16x8 xm = __builtin_bit_cast(bf16x8, pre[2][j][p]);
        bf16x8 dd;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float a = (float)ym[k] > 0.f ? (float)da[k] + (float)g2[k] : 0.f;
          dd[k] = (__bf16)a;
          if (ok) {
            const float f = (float)dd[k];
            sv[8 * p + k] += f;
            sv[16 + 8 * p + k] += f * (float)xm[k];
          }
        }
        if (ok) *reinterpret_cast<bf16x8*>(dout + 16 * p) = dd;
      }
      acc[j] = f32x16{};
    }
    // reduce-scatter over the 32 pixel lanes: at lane bit o a lane keeps the half of its
    // values whose index has that bit as its own r has, and adds the partner's copy of them;
    // afterwards lane r holds the total of value r.  Fixed order.
#pragma unroll
    for (int n = 16; n >= 1; n >>= 1) {
      const bool up = (r & n) != 0;
#pragma unroll
      for (int i = 0; i < n; ++i) {
        // (unary plus: a conditional over two array lvalues selects the ADDRESS, which turns
        // the register array into a dynamically indexed one)
        const float lo = sv[i], hi = sv[i + n];
        const float keep = up ? +hi : +lo, send = up ? +lo : +hi;
        sv[i] = keep + __shfl_xor(send, n);
      }
    }
    // value r: row r >> 4 (sum d / sum d xb), channel 16 (e >> 3) + 8h + (e & 7), e = r & 15;
    // pixel half 1 parks its total, pixel half 0 adds it to its own and stores
    const int e = r & 15, ch = wn * 32 + 16 * (e >> 3) + 8 * h + (e & 7);
    if (wm == 1) red[r >> 4][ch] = sv[0];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wm == 0) part[((int64_t)t * 2 + (r >> 4)) * N + n0 + ch] = sv[0] + red[r >> 4][ch];
  };

  int st = 0;
  int cur_tile = (int)(u0 / groups);
  // one column block: its nch stages, then its epilogue from `cur`; the NEXT block's operands
  // go into `nxt` at the first stage (outside the chunk loop: no back-edge merge to make the
  // compiler's waits for them conservative)
  auto block = [&](int t, int n0, int nt, int nn0, const PreSet& cur, PreSet& nxt) {
    bw_wait<NS - 2>();
    if (t != cur_tile) {  // workgroup-uniform: every wave is past its reads of the old tile
      load_tile(t);
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      cur_tile = t;
    }
    issue();
    prefetch(nxt, nt, nn0);
    compute(st, 0);
    ++st;
    for (int kc = 1; kc < nch; ++kc, ++st) {
      // the prefetch above is younger than this stage's DMA for the NS - 1 stages after it
      // (counted for NS - 2 of them: one stage of margin; counting fewer only waits longer)
      if (kc <= NS - 2)
        bw_wait<NS - 2 + kBwPreLoads>();
      else
        bw_wait<NS - 2>();
      issue();
      compute(st, kc);
    }
    epilogue(t, n0, cur);
  };

  load_tile(cur_tile);
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue();
  // block cursor: unit bu (group bg), column block bc; next() steps it, staying on the last
  int64_t bu = u0;
  int bg = (int)(u0 % groups), bc = 0, bt = cur_tile;
  bool more = true;
  auto next = [&]() {
    if (bc + 1 < unit_ncb(bg)) {
      ++bc;
    } else if (bu + 1 < u1) {
      ++bu, bc = 0;
      if (bg + 1 < groups) {
        ++bg;
      } else {
        bg = 0, ++bt;
      }
    } else {
      more = false;
    }
  };
  PreSet pa, pb;
  prefetch(pa, bt, (kBwGroupBlocks * bg + bc) * 64);
  while (more) {
    int t = bt, n0 = (kBwGroupBlocks * bg + bc) * 64;
    next();
    block(t, n0, bt, (kBwGroupBlocks * bg + bc) * 64, pa, pb);  // past the end: a harmless re-load
    if (!more) break;
    t = bt, n0 = (kBwGroupBlocks * bg + bc) * 64;
    next();
    block(t, n0, bt, (kBwGroupBlocks * bg + bc) * 64, pb, pa);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may outlive the workgroup's LDS
}

}  // namespace

Conv1x1BnBwdWideGeom conv1x1_bn_bwd_wide_geom(int64_t M, int64_t K, int64_t N) {
  Conv1x1BnBwdWideGeom g{};
  if (M <= 0 || K <= 0 || N <= 0 || M > (int64_t)1 << 30 || K > 1 << 20 || N > 1 << 20) return g;
  g.M = M, g.K = (int)K, g.N = (int)N;
  g.rows = (int)((M + kBwTileM - 1) / kBwTileM);
  g.groups = (int)((N / 64 + kBwGroupBlocks - 1) / kBwGroupBlocks);
  g.units = (int64_t)g.rows * g.groups;
  const bool small = K <= kBwSmallK;
  g.stages = small ? kBwSmallStages : kBwStages;
  g.lds_bytes = (small ? kBwSmallK : kBwMaxK) * 256 + g.stages * kBwStageBytes + 2 * 64 * 4;
  const int64_t resident = (int64_t)(small ? 2 : 1) * plan_cus();
  const int64_t want = g.units < resident ? g.units : resident;
  g.grid = (int)((want + 7) / 8 * 8);
  return g;
}

bool conv1x1_bn_bwd_wide_ok(const Conv1x1BnBwdWideGeom& g) {
  return g.M > 0 && g.K > 128 && g.K <= kBwMaxK && g.K % 32 == 0 && g.N >= 64 && g.N <= 4096 && g.N % 64 == 0 && g.grid > 0;
}

int conv1x1_bn_bwd_wide_tile_m() { return kBwTileM; }

bool launch_conv1x1_bn_bwd_wide(const uint16_t* dy1, const uint16_t* w, uint16_t* d, const Conv1x1BnBwdWideGeom& g,
                                const uint16_t* dy2, const uint16_t* yb, const uint16_t* xb, float* part,
                                hipStream_t s) {
  if (!conv1x1_bn_bwd_wide_ok(g) || !dy1 || !w || !d || !dy2 || !yb || !xb || !part) return false;
  const dim3 grid((unsigned)g.grid), block(kBwThreads);
  if (g.K <= kBwSmallK)
    hipLaunchKernelGGL((conv1x1_bn_bwd_wide_kernel<kBwSmallStages, kBwSmallK>), grid, block, 0, s, dy1, w, d, g.M, g.K,
                       g.N, g.groups, g.units, dy2, yb, xb, part);
  else
    hipLaunchKernelGGL((conv1x1_bn_bwd_wide_kernel<kBwStages, kBwMaxK>), grid, block, 0, s, dy1, w, d, g.M, g.K, g.N,
                       g.groups, g.units, dy2, yb, xb, part);
  return true;
}

}  // namespace rla
