// Input gradient of a FORKED pair of 1x1 NHWC bf16 convolutions reading one tensor (gfx950):
// ResNet's bottleneck conv1 (stride 1) and its downsample shortcut (stride s = 1 or 2).
//
//   dx[n][h][w][:] = bf16(dy1[n][h][w][:] . w1  +  [h % s == 0 and w % s == 0] dyd[n][h/s][w/s][:] . wd)
//
// dy1 [N, H, W, C1], dyd [N, OH, OW, Cd] (OH = (H - 1) / s + 1), w1 [C1][Cin] and wd [Cd][Cin]
// the FORWARD weights as stored.  Both GEMMs go into the same fp32 MFMA accumulators -- w1's
// 32-row chunks ascending, then wd's ascending -- and dx is stored exactly once with one
// rounding: no zero-fill, no read-modify-write, no atomics, and nothing in the order depends
// on the tile, the plan or the workgroup, so two calls under any two plans agree bitwise.
//
// Tiles.  s = 2: the work is tiled over quads (n, a, b), a < OH, b < OW -- the four input
// pixels (2a + dr, 2b + dc), as in conv3x3s2_dgrad.hip -- whose linear index IS dyd's row
// index.  A tile is 128 quads = 512 pixels x 64 channels, its 16 MFMA row blocks of 32 ordered
// by parity class (dr, dc): the four class (0, 0) blocks take both GEMMs, the twelve others
// only dy1 . w1, so no MFMA is spent on a zero contribution.  The dy1 rows of a class are
// gathered ((n H + 2a + dr) W + 2b + dc); pixels past the image at odd H / W read a clamped
// (valid) row and are not stored, as are the quads past the end of a short last tile.
// s = 1: no quads -- a tile is 512 consecutive pixels and every block takes both GEMMs
// (the concatenated-K GEMM [dy1 | dyd] . [w1 ; wd]); same kernel, second instance.
//
// Waves.  256 threads = 2 channel halves (wn) x 2 quad halves (wq): a wave owns 32 channels of
// all four classes of 64 quads (8 blocks of v_mfma_f32_32x32x16_bf16, 128 accumulators), so
// every wave does the same share of both GEMMs and one weight fragment feeds eight MFMAs in
// the dy1 stages (two in the strided stages: the strided GEMM sees a quarter of the rows,
// which is why the quad tile is this large -- at 32 quads layer4.0 would re-read ~650 KB of
// weights per 32 KB of output).  A split by class would leave the (0, 0) wave (C1 + Cd) / C1
// times the work.
//
// Data movement.  A K stage is 32 reduction rows: the weight slab [32 k][64 channels] read as
// stored -- rows of 128 B whose 16-byte pieces are XOR-swizzled by k & 7 through the DMA's
// source addresses, A fragments by ds_read_b64_tr_b16 (conv1x1_bn_bwd_wide.hip's scheme: no
// w.t().contiguous()) -- and the dy rows [4 k units][rows] x 16 B, unit-major (contiguous
// 512-byte ds_read_b128 runs), gathered by per-lane-address LDS-DMA (conv1x1s2.hip).  Stages
// go through a ring of 3 (36 KB each: 108 KB, one workgroup per CU) retired by a COUNTED vmcnt
// and one raw barrier; a dy1 stage is 9 DMA instructions per wave, a strided stage 3, and the
// wait counts the instructions of the one younger stage in flight.  The ring runs on across
// units (the issue cursor keeps its own row map, recomputed when it enters a unit); stages
// past the end of a workgroup's stream re-load the last one.
// Epilogue: round to bf16, one v_permlane32_swap per dword pair, 16-byte stores.
//
// Work split.  Persistent workgroups, min(units, plan_cus()) of them; unit u = column block
// u / tiles, tile u % tiles, workgroup b takes the contiguous range [units b / G,
// units (b + 1) / G): its consecutive units share a column block, whose (C1 + Cd) x 64
// weight slab stays in L2.
// Departures from the proposed starting point: none in the tile (128 quads x 64 channels,
// 128 accumulators); the ring is 3 deep because 4 stages of 36 KB would not leave room for
// anything else in 160 KB and the layer is not latency-bound at 9 KB per wave in flight.
// Requires Cin % 64 == 0, C1 % 32 == 0, Cd % 32 == 0, 16-byte aligned bases, N H W < 2^31 - 512
// (binding checks).  Only vector stores reach global memory.
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

constexpr int kFdThreads = 256;
constexpr int kFdQuads = 128;             // quads per tile (s = 2); a quarter of the pixels (s = 1)
constexpr int kFdRows = 4 * kFdQuads;     // pixels per tile
constexpr int kFdCols = 64;               // channels per unit
constexpr int kFdStages = 3;              // ring depth
constexpr int kFdWBytes = 32 * kFdCols * 2;                    // weight slab of a stage
constexpr int kFdStageBytes = kFdWBytes + 4 * kFdRows * 16;    // + [4 k units][512 rows] x 16 B
constexpr int kFdLdsBytes = kFdStages * kFdStageBytes;
static_assert(kFdLdsBytes <= 160 * 1024, "LDS budget");
static_assert(kFdStages == 3, "the wait counts the ONE younger stage in flight");

__device__ __forceinline__ bf16x4 fd_tr4(const uint8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(p));
}

__device__ __forceinline__ bf16x8 fd_cat8(bf16x4 lo, bf16x4 hi) {
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the oldest stage in flight landed (CNT DMA instructions of the one younger stage may still
// fly), every wave's LDS reads of the previous stage are done
template <int CNT>
__device__ __forceinline__ void fd_wait() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" ::"n"(CNT) : "memory");
}

template <int S>
__global__ __launch_bounds__(kFdThreads, 1) void conv1x1_fork_dgrad_kernel(
    const uint16_t* __restrict__ dy1, const uint16_t* __restrict__ w1, const uint16_t* __restrict__ dyd,
    const uint16_t* __restrict__ wd, uint16_t* __restrict__ dx, int H, int W, int OH, int OW, int Cin, int C1, int Cd,
    int R, int tiles, int units) {
  constexpr int NS = kFdStages;
  constexpr int RD = S == 1 ? kFdRows : kFdQuads;  // dyd rows of a stage
  constexpr int GD = RD / 64;                      // their DMA instructions per wave
  __shared__ __attribute__((aligned(16))) uint8_t ring[kFdLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wq = wave >> 1, r = lane & 31, h = lane >> 5;
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int u0 = (int)((int64_t)units * b / G), u1 = (int)((int64_t)units * (b + 1) / G);
  if (u0 >= u1) return;
  const int nk1 = C1 >> 5, nk = nk1 + (Cd >> 5);
  const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)ring;

  // Tile row (class c, slot q) of tile t.  s = 2: quad Q = 128 t + q = dyd's row, pixel
  // (2a + (c >> 1), 2b + (c & 1)) of image n; s = 1: pixel 512 t + 128 c + q, which is dyd's
  // row too.  Returns whether the pixel exists; what does not is clamped to a valid row.
  auto rowmap = [&](int t, int c, int q, int& pix, int& drow) -> bool {
    if (S == 1) {
      const int p = t * kFdRows + c * kFdQuads + q;
      const bool ok = p < R;
      pix = drow = ok ? p : R - 1;
      return ok;
    }
    int Q = t * kFdQuads + q;
    bool ok = Q < R;
    Q = ok ? Q : R - 1;
    const int n = Q / (OH * OW), rem = Q - n * (OH * OW);
    const int a = rem / OW, bb = rem - a * OW;
    int hh = 2 * a + (c >> 1), ww = 2 * bb + (c & 1);
    ok = ok && hh < H && ww < W;
    hh = hh < H ? hh : H - 1;
    ww = ww < W ? ww : W - 1;
    pix = (n * H + hh) * W + ww;
    drow = Q;
    return ok;
  };

  // ---- issue side: the stage stream over (unit, k chunk), with its own row map ----
  // dy rows: wave-instruction j covers k unit `wave`, tile rows 64 j .. +64 (class j / 2)
  int r1[8], rd[GD];
  int iu = u0, ik = 0, icb = 0, islot = 0;
  bool last_p1 = true;  // the youngest issued stage is a dy1 stage (9 DMA instructions, else 1 + GD)
  auto enter = [&](int u) {
    icb = u / tiles;
    const int t = u - icb * tiles;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int drow;
      rowmap(t, j >> 1, 64 * (j & 1) + lane, r1[j], drow);
      if (S == 1) rd[j % GD] = drow;
    }
    if (S == 2) {
#pragma unroll
      for (int j = 0; j < GD; ++j) {
        int pix;
        rowmap(t, 0, 64 * j + lane, pix, rd[j]);
      }
    }
  };
  // weight slab: this wave's instruction covers stage rows 8 wave .. +8 (lane >> 3), the row's
  // eight 16-byte pieces stored at slot piece ^ (row & 7)
  const int wl = (8 * wave + (lane >> 3)) * Cin + 8 * ((lane & 7) ^ (lane >> 3));
  auto issue = [&]() {
    const uint32_t buf = ring0 + (uint32_t)islot * kFdStageBytes;
    islot = islot + 1 == NS ? 0 : islot + 1;
    if (ik < nk1) {
      c1_dma16(w1 + (int64_t)ik * 32 * Cin + icb * kFdCols + wl, __builtin_amdgcn_readfirstlane(buf + wave * 1024));
#pragma unroll
      for (int j = 0; j < 8; ++j)
        c1_dma16(dy1 + (int64_t)r1[j] * C1 + 32 * ik + 8 * wave,
                 __builtin_amdgcn_readfirstlane(buf + kFdWBytes + (wave * kFdRows + 64 * j) * 16));
      last_p1 = true;
    } else {
      const int kk = ik - nk1;
      c1_dma16(wd + (int64_t)kk * 32 * Cin + icb * kFdCols + wl, __builtin_amdgcn_readfirstlane(buf + wave * 1024));
#pragma unroll
      for (int j = 0; j < GD; ++j)
        c1_dma16(dyd + (int64_t)rd[j] * Cd + 32 * kk + 8 * wave,
                 __builtin_amdgcn_readfirstlane(buf + kFdWBytes + (wave * RD + 64 * j) * 16));
      last_p1 = false;
    }
    if (ik + 1 < nk) {
      ++ik;
    } else if (iu + 1 < u1) {
      ++iu, ik = 0;
      enter(iu);
    }  // else: the stream's last stage again
  };

  // ---- compute side ----
  // transposed-read lane roles (conv_wgrad.hip): 16-lane group gq, lane 4q + p addresses k row
  // q, channels 4p .. 4p + 3; the two reads of a fragment are k rows rwo and rwo + 4
  const int gq = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
  const int wch = wn * 32 + 16 * (gq & 1) + 4 * tp;  // channel inside the 64-channel block
  const int rwo = 8 * (gq >> 1) + tq;                // k row inside a 16-row step
  const int aoff0 = rwo * 128 + (((wch >> 3) ^ tq) << 4) + (wch & 7) * 2;
  const int aoff1 = (rwo + 4) * 128 + (((wch >> 3) ^ (tq + 4)) << 4) + (wch & 7) * 2;
  const int boff = (64 * wq + r) * 16;

  f32x16 acc[4][2];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[c][j] = f32x16{};

  auto compute = [&](int slot, bool p1) {
    const uint8_t* buf = ring + slot * kFdStageBytes;
    const uint8_t* rb = buf + kFdWBytes + boff;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 fa = fd_cat8(fd_tr4(buf + ks * 2048 + aoff0), fd_tr4(buf + ks * 2048 + aoff1));
      if (S == 1 || p1) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                fa, *reinterpret_cast<const bf16x8*>(rb + ((2 * ks + h) * kFdRows + c * kFdQuads + 32 * j) * 16),
                acc[c][j], 0, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              fa, *reinterpret_cast<const bf16x8*>(rb + ((2 * ks + h) * RD + 32 * j) * 16), acc[0][j], 0, 0, 0);
      }
    }
  };

  // D[n][m]: lane -> pixel slot r of block (c, j); accumulator 4q + e -> channel 8q + 4h + e.
  // One v_permlane32_swap per dword of each channel-group pair (q, q + 1) gives lane h
  // channels 16p + 8h .. +8: one 16-byte store
  auto epilogue = [&](int t, int cb) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int pix, drow;
        const bool ok = rowmap(t, c, 64 * wq + 32 * j + r, pix, drow);  // lanes l and l ^ 32 share the pixel
        uint16_t* out = dx + (int64_t)pix * Cin + cb * kFdCols + wn * 32 + 8 * h;
        uint32_t v[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = (__bf16)acc[c][j][4 * q + e];
          const u32x2 pk = __builtin_bit_cast(u32x2, o);
          v[q][0] = pk[0];
          v[q][1] = pk[1];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(v[2 * p][0], v[2 * p + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(v[2 * p][1], v[2 * p + 1][1], false, false);
          const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
          if (ok) *reinterpret_cast<u32x4*>(out + 16 * p) = o;
        }
        acc[c][j] = f32x16{};
      }
  };

  enter(u0);
#pragma unroll
  for (int s = 0; s < NS - 1; ++s) issue();
  int slot = 0;
  for (int u = u0; u < u1; ++u) {
    const int cb = u / tiles, t = u - cb * tiles;
    for (int k = 0; k < nk; ++k) {
      // the one younger stage in flight is the last one issued
      if (S == 1 || last_p1)
        fd_wait<9>();
      else
        fd_wait<1 + GD>();
      issue();
      compute(slot, k < nk1);
      slot = slot + 1 == NS ? 0 : slot + 1;
    }
    epilogue(t, cb);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no DMA may outlive the workgroup's LDS
}

}  // namespace

Conv1x1ForkDgradGeom conv1x1_fork_dgrad_geom(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t C1, int64_t Cd,
                                             int64_t s) {
  Conv1x1ForkDgradGeom g{};
  const int64_t lim = int64_t(1) << 31, cmax = 1 << 20;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || C1 <= 0 || Cd <= 0 || (s != 1 && s != 2)) return g;
  if (N >= lim || H >= lim || W >= lim || Cin > cmax || C1 > cmax || Cd > cmax) return g;
  // 32-bit row indexing, with room for a short last tile's row numbers past the end
  if (N * H >= lim || N * H * W >= lim - kFdRows) return g;
  const int64_t oh = (H - 1) / s + 1, ow = (W - 1) / s + 1;
  const int64_t rows = s == 1 ? N * H * W : N * oh * ow, per = s == 1 ? kFdRows : kFdQuads;
  const int64_t tiles = (rows + per - 1) / per, cols = Cin / kFdCols;
  if (tiles * (cols > 0 ? cols : 1) >= lim) return g;
  g.N = (int)N, g.H = (int)H, g.W = (int)W, g.Cin = (int)Cin, g.C1 = (int)C1, g.Cd = (int)Cd, g.s = (int)s;
  g.OH = (int)oh, g.OW = (int)ow, g.rows = (int)rows, g.tiles = (int)tiles, g.cols = (int)cols;
  g.units = (int)(tiles * cols);
  g.grid = g.units < plan_cus() ? g.units : plan_cus();
  return g;
}

bool conv1x1_fork_dgrad_ok(const Conv1x1ForkDgradGeom& g) {
  return g.N > 0 && g.Cin >= 64 && g.Cin <= 1024 && g.Cin % kFdCols == 0 && g.C1 % 32 == 0 && g.C1 <= 512 &&
         g.Cd % 32 == 0 && g.Cd <= 2048 && g.grid > 0;
}

int conv1x1_fork_dgrad_tile_rows(int s) { return s == 1 ? kFdRows : kFdQuads; }
int conv1x1_fork_dgrad_stages() { return kFdStages; }
int conv1x1_fork_dgrad_lds_bytes() { return kFdLdsBytes; }

bool launch_conv1x1_fork_dgrad(const uint16_t* dy1, const uint16_t* w1, const uint16_t* dyd, const uint16_t* wd,
                               uint16_t* dx, const Conv1x1ForkDgradGeom& g, hipStream_t stream) {
  if (!conv1x1_fork_dgrad_ok(g) || !dy1 || !w1 || !dyd || !wd || !dx) return false;
  const dim3 grid((unsigned)g.grid), block(kFdThreads);
  if (g.s == 1)
    hipLaunchKernelGGL(conv1x1_fork_dgrad_kernel<1>, grid, block, 0, stream, dy1, w1, dyd, wd, dx, g.H, g.W, g.OH, g.OW,
                       g.Cin, g.C1, g.Cd, g.rows, g.tiles, g.units);
  else
    hipLaunchKernelGGL(conv1x1_fork_dgrad_kernel<2>, grid, block, 0, stream, dy1, w1, dyd, wd, dx, g.H, g.W, g.OH, g.OW,
                       g.Cin, g.C1, g.Cd, g.rows, g.tiles, g.units);
  return true;
}

}  // namespace rla
