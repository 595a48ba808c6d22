// 3x3 / stride 2 / pad 1 NHWC bf16 convolution forward on the MFMA units (gfx950):
//
//   y[n][oh][ow][co] = sum over r, s, ci of x[n][2 oh + r - 1][2 ow + s - 1][ci] * w[co][r][s][ci]
//
// with OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1.  ResNet-50's three downsample conv2
// layers (layer2/3/4.0.conv2: 56/128, 28/256, 14/512 as input width / Cin), each the
// same 29.6 GFLOP at batch 128 as a stride-1 conv2.  This file is the forward; the input
// gradient of these layers is conv3x3s2_dgrad.hip's (tiled over quads of input pixels), the
// weight gradient conv_wgrad.hip's.
//
// The structure is conv3x3.hip's (read that header first): implicit GEMM
// D[co][m] = W[co][(tap, ci)] . X[(tap, ci)][m] over m = output pixel with
// v_mfma_f32_32x32x16_bf16 (A = weights, B = pixels), the reduction in chunks of 16
// input channels, a chunk's x HALO image and 9 x 64 weight rows staged in LDS, two LDS
// buffers, kS2Depth register sets in flight, one barrier per chunk, unconditional
// clamped loads, persistent workgroups: workgroup g owns output-channel block
// g % tiles_n and the (g / tiles_n)-th of wpb equal contiguous OUTPUT-pixel ranges
// (conv3x3_wpb over plan_cus(); block g runs on XCD g % 8: the channel blocks of one
// pixel range sit on different XCDs, and with tiles_n = 8 each XCD holds one weight
// block, as in conv3x3.hip), tiled from its own start with a shorter last tile.  A
// pixel is one B column of every MFMA and its chunks and taps run in a fixed order, so
// y does not depend on the tile or workgroup a pixel lands in.
//
// What stride 2 changes:
//   * the halo.  Output row oh reads padded input rows 2 oh .. 2 oh + 2 (padded = input
//     + 1) and every column: ~4 input pixels per output pixel, four times the stride-1
//     halo for the same tile.  The virtual padded image is [n][2 OH + 1][2 OW + 1]: for
//     even H (W) that is H + 1 (W + 1) -- the bottom (right) padding is never read and
//     has no row (column); for odd sizes it is H + 2 (W + 2) and the last one is zeros.
//     Neighbouring output rows share one halo row, the last row of image n and the
//     first of image n + 1 share none: virtual row v = n (2 OH + 1) + 2 oh + r.
//   * the tile.  LDS per buffer = halo + weights at 48-byte rows (16 channels + 16 B
//     pad).  A 256-pixel tile at 56x56 input touches up to 11 output rows = 23 halo
//     rows x 57 columns x 48 B = 62.9 KB; two of them and two 27.6 KB weight images are
//     181 KB > 160 KB.  So the tile is 128 output pixels x 64 channels: wave w owns
//     pixels [32 w, 32 w + 32) x all 64 channels = 2 MFMA blocks.  A tile that touches R
//     output rows and crosses X image boundaries needs 2 R + 1 + X halo rows.  Worst
//     ResNet case: 56x56 input, a full tile that starts in the last output row of an
//     image at column >= 13 and runs into the next image: R = 6, X = 1, 14 x 57 = 798
//     halo entries (inside one image: 13 x 57 = 741; 28x28 input: R <= 11, X <= 1,
//     24 x 29 = 696; 14x14: R <= 20, X <= 3, 44 x 15 = 660).  The buffer holds
//     kS2MaxNX * 128 = 896 entries (43,008 B) + 640 weight rows (30,720 B; 576 used, the
//     surplus pieces of the last store round land in the rest) = 73,728 B, two buffers
//     147,456 B <= 160 KB.  The ST reduction image (66,560 B) reuses them.  The price
//     of the small tile: 3 ds_read_b128 per 2 MFMAs and wave (the stride-1 kernel's
//     256-pixel tile has 4 per 4), i.e. 4 waves x 27 KB per chunk; at the 256 B/clk of
//     conflict-free ds_read_b128 that is ~430 clk against 576 clk of MFMA, so by this
//     model the LDS reads hide behind the MFMAs.  Measured (batch 128, MI355X) the
//     kernel is far from either: 110-123 us per ResNet layer = 240-270 TFLOP/s, ~4,500
//     clk per stage.  A stage moves ~47 KB per workgroup for 2.4 MFLOP (the stride-1
//     512-pixel tile: 38 KB for 9.4) in 12 scattered 16-byte loads per thread that each
//     use 32 B of a 128-byte line: the global -> LDS path is the suspect, not the LDS.
//     Issuing two chunks' loads back to back (to meet the line in L1) measured slower
//     (130 us); a larger tile needs another LDS plan (docs/resnet50.md).
//   * bank conflicts.  Consecutive output pixels read every SECOND halo column; in a
//     plain [2 OW + 1] row that is a 96-byte lane stride and a ds_read_b128 lane group
//     (16 lanes) folds onto 8 distinct 16-byte slots of the 256-byte bank row: 2-way.
//     The halo row is therefore staged split by column parity: [OW + 1 even padded
//     columns 0, 2, .. 2 OW][OW odd padded columns 1, 3, .. 2 OW - 1].  Tap s = 0 reads
//     even entry ow, s = 2 even entry ow + 1, s = 1 odd entry ow: consecutive pixels of
//     one output row are consecutive 48-byte entries again (3 is odd: 16 lanes land on
//     16 distinct slots), conflict-free as in conv3x3.hip.  Where a block of 32 pixels
//     wraps into the next output row the address jumps by two halo rows minus OW entries
//     and the two parts may share slots (at most 2-way, the run-time-shape stride-1
//     layout's cost too); there are no compile-time-shape instances yet that could pad
//     it away.
// ST: the next BatchNorm's partial sums of the bf16-rounded output, exactly as
// conv3x3.hip ST: per-lane register sums over all tiles, one fixed-order LDS reduction
// into row g / tiles_n of part [wpb][2][Cout]; no atomics.  Every row owns pixels:
// conv3x3_wpb keeps ranges of at least 32 and conv3x3s2_ok refuses wpb > pixels.
// Requires Cin % 16 == 0, Cout % 64 == 0, 16-byte aligned bases and a halo of at most
// 896 entries per tile, (2 R + 1 + X) (2 OW + 1) as above over the tiles of the actual
// partition (conv3x3s2_ok): every batch size at ResNet's three shapes; an output wider
// than 28 only where the ranges are short enough, e.g. three rows of OW <= 148.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

namespace rla {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kS2Threads = 256;
constexpr int kS2TM = 128;      // output pixels per workgroup tile (32 per wave)
constexpr int kS2TN = 64;       // output channels per workgroup tile
constexpr int kS2KC = 16;       // reduction channels per chunk
constexpr int kS2Row = 24;      // bf16 per halo / weight row: 16 channels + 8 pad (48 B)
constexpr int kS2Depth = 3;     // register sets (stages in flight from HBM / L2)
constexpr int kS2MaxNX = 7;     // halo pieces (16 B) per thread and chunk
constexpr int kS2WPieces = 9 * kS2TN * 2;
constexpr int kS2NW = (kS2WPieces + kS2Threads - 1) / kS2Threads;
constexpr int kS2XElems = kS2MaxNX * kS2Threads / 2 * kS2Row;
constexpr int kS2WElems = kS2NW * kS2Threads / 2 * kS2Row;
constexpr int kS2BufElems = kS2XElems + kS2WElems;
static_assert(2 * kS2BufElems * 2 <= 160 * 1024, "two LDS buffers fit the CU's 160 KiB");
static_assert(2 * kS2BufElems * 2 >= 4 * 32 * 2 * 65 * 4, "ST reduction image fits the halo buffers");

struct S2Set {
  u32x4 x[kS2MaxNX], w[kS2NW];
  uint32_t ok;  // bit i: x[i] is an in-image pixel (else zero padding)
};

template <bool ST>
__global__ __launch_bounds__(kS2Threads) void conv3x3s2_kernel(const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ w,
                                                               uint16_t* __restrict__ y, Conv3x3S2Geom g,
                                                               float* __restrict__ part) {
  constexpr int NX = kS2MaxNX, BE = kS2BufElems, XE = kS2XElems, DEPTH = kS2Depth;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int WP = 2 * g.OW + 1, HP = 2 * g.OH + 1;  // the virtual padded image
  const int RS = WP * kS2Row;                      // halo row stride (elements)
  const int odd0 = g.OW + 1;                       // first odd-column entry of a halo row
  const int64_t M = (int64_t)g.N * g.OH * g.OW;
  const int ohw = g.OH * g.OW;
  const int tiles_n = g.Cout / kS2TN;
  if ((int)blockIdx.x >= g.wpb * tiles_n) return;  // (uniform)
  const int nblk = (int)blockIdx.x % tiles_n, jr = (int)blockIdx.x / tiles_n;
  const int co0 = nblk * kS2TN;
  // this workgroup's output pixels (M < 2^31 by conv3x3s2_ok: 32-bit pixel indices from here on)
  const int p_lo = (int)(M * jr / g.wpb), p_hi = (int)(M * (jr + 1) / g.wpb);
  const int ntiles = (int)((p_hi - p_lo + kS2TM - 1) / kS2TM);
  if (ntiles == 0) return;  // (never: conv3x3s2_ok requires wpb <= M)
  const int nchunks = g.Cin / kS2KC;
  const int nst = ntiles * nchunks;
  const int xpieces = g.vrows * WP * 2;  // 16-byte pieces of a chunk's halo image

  // this workgroup's tile of stream stage `st` (clamped: stages past the end re-load the last one)
  auto tile_of = [&](int st, int* chunk) {
    const int sc = st < nst ? st : nst - 1;
    const int i = sc / nchunks;
    *chunk = sc - i * nchunks;
    return i;
  };
  // tile i: output pixels [m0, m_end); v0: its first virtual halo row
  auto tile_org = [&](int tile, int* m0, int* v0, int* m_end = nullptr) {
    *m0 = p_lo + tile * kS2TM;
    if (m_end) *m_end = *m0 + kS2TM < p_hi ? *m0 + kS2TM : p_hi;
    const int n0 = *m0 / ohw, oh0 = (*m0 - n0 * ohw) / g.OW;
    *v0 = n0 * HP + 2 * oh0;
  };

  // load-side tile state: byte offsets of this thread's pieces (without the chunk's
  // channel offset) and their validity, once per tile
  int ld_tile = -1;
  uint32_t xoff[NX], woff[kS2NW];
  uint32_t xok = 0u;
  auto load_geom = [&](int tile) {
    int m0;
    int v0;
    tile_org(tile, &m0, &v0);
    xok = 0u;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int p = tid + i * kS2Threads;
      const int pc = p < xpieces ? p : xpieces - 1;
      const int e = pc >> 1, h = pc & 1;
      const int vr = e / WP, q = e - vr * WP;
      // entry q of a halo row: even padded column 2 q, or odd padded column 2 (q - odd0) + 1
      const int pcol = q < odd0 ? 2 * q : 2 * (q - odd0) + 1;
      const int v = v0 + vr;
      const int n = v / HP, ih = v - n * HP - 1, iw = pcol - 1;
      const bool ok = p < xpieces && n < g.N && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W;
      const int nc = n < g.N ? n : g.N - 1;
      const int ihc = ih < 0 ? 0 : (ih >= g.H ? g.H - 1 : ih), iwc = iw < 0 ? 0 : (iw >= g.W ? g.W - 1 : iw);
      xoff[i] = (uint32_t)(((nc * g.H + ihc) * g.W + iwc) * g.Cin + h * 8) * 2u;
      xok |= ok ? (1u << i) : 0u;
    }
#pragma unroll
    for (int i = 0; i < kS2NW; ++i) {
      const int p = tid + i * kS2Threads;
      const int pc = p < kS2WPieces ? p : kS2WPieces - 1;
      const int h = pc & 1, rest = pc >> 1, co = rest % kS2TN, tap = rest / kS2TN;
      woff[i] = (uint32_t)(((co0 + co) * 9 + tap) * g.Cin + h * 8) * 2u;
    }
  };
  auto load = [&](S2Set& st, int stage) {
    int cc;
    const int tile = tile_of(stage, &cc);
    if (tile != ld_tile) {  // uniform: the stage stream crossed into a new tile
      load_geom(tile);
      ld_tile = tile;
    }
    const uint32_t ci0b = (uint32_t)(cc * kS2KC) * 2u;
    st.ok = xok;
    const char* xc = reinterpret_cast<const char*>(x);
    const char* wc = reinterpret_cast<const char*>(w);
#pragma unroll
    for (int i = 0; i < NX; ++i) st.x[i] = *reinterpret_cast<const u32x4*>(xc + (xoff[i] + ci0b));
#pragma unroll
    for (int i = 0; i < kS2NW; ++i) st.w[i] = *reinterpret_cast<const u32x4*>(wc + (woff[i] + ci0b));
  };
  auto store = [&](const S2Set& st, int buf) {
    __bf16* X = lds + buf * BE;
    __bf16* Wt = X + XE;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NX; ++i) {  // p >= xpieces: an entry past the image, never read
      const int p = tid + i * kS2Threads;
      *reinterpret_cast<u32x4*>(X + (p >> 1) * kS2Row + (p & 1) * 8) = (st.ok >> i) & 1u ? st.x[i] : z;
    }
#pragma unroll
    for (int i = 0; i < kS2NW; ++i) {
      const int p = tid + i * kS2Threads;  // pieces past 9 taps land in unused rows
      *reinterpret_cast<u32x4*>(Wt + (p >> 1) * kS2Row + (p & 1) * 8) = st.w[i];
    }
  };

  const int kg = (lane >> 5) * 8;  // k-group: channels 8 (lane / 32) .. + 7 of the chunk
  int bpos = 0;  // this lane's pixel as an LDS element offset of tap (0, 0)
  auto set_tile = [&](int tile) {
    int m0, m_end;
    int v0;
    tile_org(tile, &m0, &v0, &m_end);
    int m = m0 + wave * 32 + (lane & 31);
    if (m >= m_end) m = m_end - 1;  // past the tile: a duplicate, never stored
    const int n = m / ohw, rem = m - n * ohw;
    const int oh = rem / g.OW, ow = rem - oh * g.OW;
    bpos = (n * HP + 2 * oh - v0) * RS + ow * kS2Row + kg;
  };

  f32x16 acc[2];
  auto zero = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
  };

  // tap t + 1's fragments are read while tap t's MFMAs run (one wave per SIMD: nothing
  // else hides the LDS latency)
  auto fetch = [&](const __bf16* X, const __bf16* Wt, int tap, bf16x8 (&fa)[2], bf16x8& fb) {
    const int r = tap / 3, s = tap - (tap / 3) * 3;
    // s = 0: even entry ow; s = 1: odd entry ow; s = 2: even entry ow + 1
    const int toff = r * RS + (s == 0 ? 0 : (s == 1 ? odd0 : 1)) * kS2Row;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      fa[i] = *reinterpret_cast<const bf16x8*>(Wt + (tap * kS2TN + i * 32 + (lane & 31)) * kS2Row + kg);
    fb = *reinterpret_cast<const bf16x8*>(X + bpos + toff);
  };
  auto compute = [&](int buf) {
    const __bf16* X = lds + buf * BE;
    const __bf16* Wt = X + XE;
    bf16x8 fa[2][2], fb[2];
    fetch(X, Wt, 0, fa[0], fb[0]);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int cur = tap & 1;
      if (tap + 1 < 9) fetch(X, Wt, tap + 1, fa[cur ^ 1], fb[cur ^ 1]);
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of this tap's MFMAs
#pragma unroll
      for (int i = 0; i < 2; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[cur], acc[i], 0, 0, 0);
    }
  };

  // ST: this lane's channel sums [i][4 q + e] (channel i 32 + 8 q + 4 (lane >> 5) + e)
  float bs[2][16], bq[2][16];
  if constexpr (ST) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) bs[i][k] = bq[i][k] = 0.f;
  }

  // D[co][m]: lane -> pixel (lane & 31); accumulator k -> channel
  // (k & 3) + 8 (k >> 2) + 4 (lane >> 5) of block i
  auto epilogue = [&](int tile) {
    int m0, m_end;
    int v0;
    tile_org(tile, &m0, &v0, &m_end);
    const int m = m0 + wave * 32 + (lane & 31);
    // lanes l and l ^ 32 hold the same pixel; a v_permlane32_swap per dword of each
    // channel-group pair gives lane half (lane >> 5) 8 consecutive channels: 16-byte stores
    const bool ok = m < m_end;
    uint16_t* yo = y + (int64_t)(ok ? m : 0) * g.Cout + co0 + 8 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      uint32_t v[4][2];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bf16x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (__bf16)acc[i][4 * q + e];
        if constexpr (ST) {
          if (ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float f = (float)b[e];  // the statistics of what BatchNorm reads
              bs[i][4 * q + e] += f;
              bq[i][4 * q + e] = __builtin_fmaf(f, f, bq[i][4 * q + e]);
            }
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
        if (ok) *reinterpret_cast<u32x4*>(yo + 32 * i + 16 * p) = o;
      }
    }
  };

  // stage k of the stream: global -> register set k % DEPTH -> LDS buffer k & 1
  // (conv3x3.hip's pipeline: set (it + 1) % DEPTH goes to the buffer the previous
  // iteration finished reading and is reloaded with stage it + 1 + DEPTH)
  auto step = [&](int it, int buf, S2Set& nxt) {
    int cc;
    const int tile = tile_of(it, &cc);
    if (cc == 0) {
      set_tile(tile);
      zero();
    }
    compute(buf);
    store(nxt, buf ^ 1);
    __syncthreads();
    load(nxt, it + 1 + DEPTH);
    if (cc == nchunks - 1) epilogue(tile);
  };
  S2Set sets[DEPTH];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(sets[d], d);
  store(sets[0], 0);
  __syncthreads();
  load(sets[0], DEPTH);
  // unrolled by 2 DEPTH: the register set ((it + 1) % DEPTH) and the LDS buffer (it & 1)
  // of every step are static
  for (int it = 0; it < nst; it += 2 * DEPTH) {
#pragma unroll
    for (int d = 0; d < 2 * DEPTH; ++d) {
      if (it + d >= nst) break;  // uniform
      step(it + d, d & 1, sets[(d + 1) % DEPTH]);
    }
  }
  if constexpr (ST) {
    // [wave][pixel lane][stat][64 channels], rows padded to 65 floats; the halo buffers
    // are dead after the last stage
    constexpr int kSR = 65;
    float* red = reinterpret_cast<float*>(lds);
    __syncthreads();
    const int row = (wave * 32 + (lane & 31)) * 2;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int co = i * 32 + 8 * (k >> 2) + 4 * (lane >> 5) + (k & 3);
        red[row * kSR + co] = bs[i][k];
        red[(row + 1) * kSR + co] = bq[i][k];
      }
    __syncthreads();
    if (tid < 2 * kS2TN) {  // (stat, channel): 128 rows in a fixed order
      const int st = tid >> 6, c = tid & 63;
      float a = 0.f;
      for (int r = 0; r < 4 * 32; ++r) a += red[(2 * r + st) * kSR + c];
      part[((int64_t)jr * 2 + st) * g.Cout + co0 + c] = a;
    }
  }
}

}  // namespace

Conv3x3S2Geom conv3x3s2_geom(int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout) {
  if (!conv3x3_args_ok(N, H, W, Cin, Cout)) return Conv3x3S2Geom{};
  Conv3x3S2Geom g{(int)N, (int)H, (int)W, (int)Cin, (int)Cout, (int)((H - 1) / 2 + 1), (int)((W - 1) / 2 + 1), 0, 0};
  g.wpb = conv3x3_wpb(g.N, g.OH, g.OW, g.Cout);
  g.vrows = conv3x3_cached_vrows(2, g.N, g.H, g.W, kS2TM, g.wpb, [&g] { return conv3x3s2_vrows(g); });
  return g;
}

int conv3x3s2_vrows(const Conv3x3S2Geom& g) {
  // the most virtual halo rows any tile of the partition touches; stops early once the
  // halo cannot fit (the answer is then only "too many")
  const int64_t M = (int64_t)g.N * g.OH * g.OW;
  const int ohw = g.OH * g.OW, HP = 2 * g.OH + 1, WP = 2 * g.OW + 1;
  const int cap = kS2MaxNX * kS2Threads / 2 / WP;  // rows the halo buffer holds
  int best = 0;
  for (int j = 0; j < g.wpb && best <= cap; ++j) {
    const int64_t lo = M * j / g.wpb, hi = M * (j + 1) / g.wpb;
    for (int64_t m0 = lo; m0 < hi && best <= cap; m0 += kS2TM) {
      const int64_t m1 = (m0 + kS2TM < hi ? m0 + kS2TM : hi) - 1;
      const int n0 = (int)(m0 / ohw), oh0 = (int)((m0 % ohw) / g.OW);
      const int n1 = (int)(m1 / ohw), oh1 = (int)((m1 % ohw) / g.OW);
      const int rows = (n1 * HP + 2 * oh1 + 2) - (n0 * HP + 2 * oh0) + 1;
      if (rows > best) best = rows;
    }
  }
  return best;
}

int conv3x3s2_pieces_per_thread(const Conv3x3S2Geom& g) {
  return (int)(((int64_t)g.vrows * (2 * g.OW + 1) * 2 + kS2Threads - 1) / kS2Threads);
}

int conv3x3s2_tm() { return kS2TM; }
int conv3x3s2_nx() { return kS2MaxNX; }

bool conv3x3s2_ok(const Conv3x3S2Geom& g) {
  // 32-bit byte offsets into x and w, 32-bit virtual rows; the halo of every tile fits the buffer
  return g.N > 0 && g.H > 0 && g.W > 0 && g.Cin > 0 && g.Cout > 0 && g.Cin % kS2KC == 0 && g.Cout % kS2TN == 0 &&
         g.OH == (g.H - 1) / 2 + 1 && g.OW == (g.W - 1) / 2 + 1 && g.vrows > 0 && g.wpb > 0 &&
         g.wpb <= (int64_t)g.N * g.OH * g.OW &&
         (int64_t)g.vrows * (2 * g.OW + 1) <= kS2MaxNX * kS2Threads / 2 &&
         (int64_t)g.N * (2 * g.OH + 1) < (1ll << 30) &&
         (int64_t)g.N * g.H * g.W * g.Cin < (1ll << 31) && (int64_t)g.N * g.OH * g.OW * g.Cout < (1ll << 31) &&
         (int64_t)g.Cin * 9 * g.Cout < (1ll << 31);
}

bool launch_conv3x3s2(const uint16_t* x, const uint16_t* w, uint16_t* y, const Conv3x3S2Geom& g, hipStream_t st,
                      float* part) {
  if (!conv3x3s2_ok(g)) return false;
  // persistent: one workgroup per (output-pixel range, output-channel block)
  const dim3 grid((unsigned)(g.wpb * (g.Cout / kS2TN)));
  if (part) {
    hipLaunchKernelGGL((conv3x3s2_kernel<true>), grid, dim3(kS2Threads), 0, st, x, w, y, g, part);
  } else {
    hipLaunchKernelGGL((conv3x3s2_kernel<false>), grid, dim3(kS2Threads), 0, st, x, w, y, g, part);
  }
  return true;
}

}  // namespace rla
