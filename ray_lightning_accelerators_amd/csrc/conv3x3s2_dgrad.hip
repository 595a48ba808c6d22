// Input gradient of the 3x3 / stride 2 / pad 1 NHWC bf16 convolution on the MFMA units (gfx950):
//
//   dx[n][ih][iw][ci] = sum over (r, s, co) of dy[n][oh][ow][co] * w[co][r][s][ci]
//                       with 2 oh + r - 1 = ih and 2 ow + s - 1 = iw
//
// dy [N, OH, OW, Cr], w the FORWARD weight [Cr][3][3][Co] as it lies in memory (no re-layout
// kernel), dx [N, H, W, Co]; OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1.  The names are
// conv3x3_dgrad_bn's: Cr is the layer's output channels (the reduction axis), Co its input
// channels.  H and W are arguments: OH does not determine H.  ResNet-50's three downsample
// conv2 layers (layer2/3/4.0.conv2); csrc/conv3x3s2.hip is their forward.
//
// Decomposition.  The work is tiled over QUADS: quad (n, a, b), a < OH, b < OW, is the four
// input pixels (2 a + dr, 2 b + dc), dr, dc in {0, 1}.  There are N OH OW quads and every
// input pixel lies in exactly one, so dx is written exactly once: no zero-fill, no atomics.
// Extend dy by one zero row below and one zero column right of each image and let
// A = dy(a, b), B = dy(a, b + 1), C = dy(a + 1, b), D = dy(a + 1, b + 1).  An input row 2 a
// is reached by r = 1 only (oh = a), a row 2 a + 1 by r = 0 (oh = a + 1) and r = 2 (oh = a);
// the same for columns, so with W[r][s] . X = sum over co of w[co][r][s][ci] X[co]
//
//   class 0: dx(2 a    , 2 b    ) = W[1][1] A
//   class 1: dx(2 a    , 2 b + 1) = W[1][0] B + W[1][2] A
//   class 2: dx(2 a + 1, 2 b    ) = W[0][1] C + W[2][1] A
//   class 3: dx(2 a + 1, 2 b + 1) = W[0][0] D + W[0][2] C + W[2][0] B + W[2][2] A
//
// 9 MFMA taps per quad, chunk and channel block -- the forward's FLOPs with none wasted (a
// zero-inserted stride-1 convolution would spend 4x) -- into four accumulator sets, one per
// parity class, from only FOUR distinct B fragments per quad block and chunk.  Tap
// t = 3 r + s feeds class 2 (r != 1) + (s != 1) from fragment 2 (r == 0) + (s == 0) of
// (A, B, C, D); the taps run in the order 0 .. 8.  Pixels 2 a + 1 >= H or 2 b + 1 >= W (odd
// sizes) are computed and not stored.
//
// Structure: conv3x3s2.hip's and conv3x3.hip FLIP's (read those headers first).  Implicit
// GEMM D[ci][quad] = W[ci][(tap, co)] . DY[(tap, co)][quad] with v_mfma_f32_32x32x16_bf16
// (A = weights, B = quads), the reduction in chunks of 16 Cr channels.  A chunk's weights
// are staged in conv3x3.hip's FLIP image [tap][k][ci] (kDgFRow-element rows) and read as A
// fragments by transposed LDS reads (ds_read_b64_tr_b16); the taps are NOT mirrored here
// (LDS tap t is w's tap t: the parity classes above already name the forward's taps).  The
// dy halo of a tile is the virtual image [n][OH + 1][OW + 1] whose extra row and column ARE
// the zeros above: virtual row v = n (OH + 1) + a, quad (n, a, b) reads rows v, v + 1 and
// columns b, b + 1; neighbouring quad rows share a halo row, the last row of image n and the
// first of image n + 1 share none.  Rows are 48 B (16 channels + 16 B pad): consecutive quads
// are consecutive entries, 16 lanes of a ds_read_b128 land on 16 distinct 16-byte slots.
// Two LDS buffers, kDgDepth register sets in flight, one barrier per chunk, unconditional
// clamped loads.  Persistent workgroups: workgroup g owns Co block g % (Co / 64) and the
// (g / (Co / 64))-th of wpb equal contiguous QUAD ranges (conv3x3_wpb(N, OH, OW, Co) over
// plan_cus()), tiled from its own start with a shorter last tile.  The epilogue is the
// forward's (v_permlane32_swap, 16-byte stores), once per class.  A quad is one B column of
// every MFMA and its chunks and taps run in a fixed order, so dx does not depend on the
// tile, the workgroup or the plan.
//
// Arithmetic (per workgroup of 4 waves; wave w owns quads [32 JB w, 32 JB (w + 1)) of a
// tile of 128 JB quads x 64 Co channels):
//   * accumulators: 4 classes x JB quad blocks x 2 channel blocks x 16 fp32 per lane = 128
//     at JB = 1, 256 at JB = 2 (the whole AGPR half of the unified 512-entry file);
//   * halo buffer: kDgNX = 4 pieces per thread = 512 entries (24,576 B).  A tile that
//     touches R quad rows and crosses X image boundaries needs R + 1 + X halo rows of OW + 1
//     entries.  256-quad tiles: OW = 28: at most 13 x 29 = 377; OW = 14: 23 x 15 = 345;
//     OW = 7: 45 x 8 = 360.  128-quad tiles need about half;
//   * weights: 9 taps x 16 k x 96 x 2 B = 27,648 B used of 160 rows (30,720 B; the surplus
//     pieces of the last store round land in the rest).  One buffer 55,296 B, two 110,592 B
//     <= 160 KB;
//   * a 256-quad stage moves 256 x 32 B of dy + halo (~12 KB) + 18 KB of weights = ~30 KB
//     for 9 x 256 x 64 x 16 x 2 = 4.7 MFLOP: about 4x the forward's FLOP per byte (47 KB for
//     2.4 MFLOP); per chunk and wave 4 JB ds_read_b128 + 36 ds_read_b64_tr_b16 for 18 JB MFMAs.
// The tile (kDgJB) is chosen from the compiler's register report
// (profiles/r12_conv3x3s2_dgrad/resource_usage.md): the 256-quad tile spills at every
// pipeline depth (256 accumulators leave 256 registers for three register sets of 9 pieces,
// 32 B-fragment and 16 A-fragment registers and the per-tile tables: 712-980 B of scratch
// per lane), so the tile is 128 quads x 64 channels, JB = 1: 256 VGPRs + 140-175 AGPRs, no
// scratch, no spills.  Its stage moves ~24 KB for 2.4 MFLOP, twice the forward's ratio.
// ResNet's worst 128-quad halos are 232 / 195 / 192 entries (OW = 28 / 14 / 7, any batch size
// on 256 CUs) = 2 pieces per thread, so the kernel is instantiated for NX = 2, 3 and 4 halo
// pieces per thread and the launch takes the smallest that fits (conv3x3s2_dgrad_nx): a
// thread then issues 2 + 5 instead of 4 + 5 16-byte loads and LDS stores per stage.
// Requires Cr % 16 == 0, Co % 64 == 0, 16-byte aligned bases, 32-bit offsets and a halo of
// at most 512 entries for every tile of the actual partition (conv3x3s2_dgrad_ok): every
// batch size at ResNet's three shapes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "kernels.h"

namespace rla {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#ifndef RLA_S2DG_JB  // (the register report compiles both tiles and several depths)
#define RLA_S2DG_JB 1
#endif
constexpr int kDgThreads = 256;
constexpr int kDgJB = RLA_S2DG_JB;  // quad blocks of 32 per wave
constexpr int kDgTQ = 128 * kDgJB;  // quads per workgroup tile
constexpr int kDgTN = 64;           // dx channels per workgroup tile
constexpr int kDgKC = 16;           // reduction channels per chunk
constexpr int kDgRow = 24;          // bf16 per halo row: 16 channels + 8 pad (48 B)
constexpr int kDgFRow = 96;         // weight rows: 64 dx channels + 32 pad (conv3x3.hip's FLIP image)
#ifndef RLA_S2DG_DEPTH
#define RLA_S2DG_DEPTH 3
#endif
constexpr int kDgDepth = RLA_S2DG_DEPTH;  // register sets (stages in flight from HBM / L2)
constexpr int kDgNX = 4;            // halo pieces (16 B) per thread and chunk the buffer holds; instances: 2, 3, 4
constexpr int kDgWPieces = 9 * kDgKC * (kDgTN / 8);
constexpr int kDgNW = (kDgWPieces + kDgThreads - 1) / kDgThreads;
constexpr int kDgXElems = kDgNX * kDgThreads / 2 * kDgRow;
constexpr int kDgWElems = kDgNW * kDgThreads / 8 * kDgFRow;
constexpr int kDgBufElems = kDgXElems + kDgWElems;
static_assert(kDgJB == 1 || kDgJB == 2, "128- or 256-quad tiles");
static_assert(2 * kDgBufElems * 2 <= 160 * 1024, "two LDS buffers fit the CU's 160 KiB");

__device__ __forceinline__ bf16x4 tr4(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(p));
}

template <int NX>
struct DgSet {
  u32x4 x[NX], w[kDgNW];
  uint32_t ok;  // bit i: x[i] is an in-image dy pixel (else the zero row / column)
};

template <int NX>
__global__ __launch_bounds__(kDgThreads) void conv3x3s2_dgrad_kernel(const uint16_t* __restrict__ dy,
                                                                     const uint16_t* __restrict__ w,
                                                                     uint16_t* __restrict__ dx,
                                                                     Conv3x3S2DgradGeom g) {
  constexpr int BE = kDgBufElems, XE = kDgXElems, DEPTH = kDgDepth, JB = kDgJB, TQ = kDgTQ;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * BE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int WP = g.OW + 1, HP = g.OH + 1;  // the virtual dy image
  const int RS = WP * kDgRow;              // halo row stride (elements)
  const int64_t Q = (int64_t)g.N * g.OH * g.OW;
  const int ohw = g.OH * g.OW;
  const int tiles_n = g.Co / kDgTN;
  if ((int)blockIdx.x >= g.wpb * tiles_n) return;  // (uniform)
  const int nblk = (int)blockIdx.x % tiles_n, jr = (int)blockIdx.x / tiles_n;
  const int co0 = nblk * kDgTN;
  // this workgroup's quads (Q < 2^31 by conv3x3s2_dgrad_ok: 32-bit quad indices from here on)
  const int q_lo = (int)(Q * jr / g.wpb), q_hi = (int)(Q * (jr + 1) / g.wpb);
  const int ntiles = (q_hi - q_lo + TQ - 1) / TQ;
  if (ntiles == 0) return;  // (never: conv3x3s2_dgrad_ok requires wpb <= Q)
  const int nchunks = g.Cr / kDgKC;
  const int nst = ntiles * nchunks;
  const int xpieces = g.vrows * WP * 2;  // 16-byte pieces of a chunk's halo image

  // this workgroup's tile of stream stage `st` (clamped: stages past the end re-load the last one)
  auto tile_of = [&](int st, int* chunk) {
    const int sc = st < nst ? st : nst - 1;
    const int i = sc / nchunks;
    *chunk = sc - i * nchunks;
    return i;
  };
  // tile i: quads [q0, q_end); v0: its first virtual halo row
  auto tile_org = [&](int tile, int* q0, int* v0, int* q_end = nullptr) {
    *q0 = q_lo + tile * TQ;
    if (q_end) *q_end = *q0 + TQ < q_hi ? *q0 + TQ : q_hi;
    const int n0 = *q0 / ohw, a0 = (*q0 - n0 * ohw) / g.OW;
    *v0 = n0 * HP + a0;
  };

  // the weight pieces are the workgroup's own: piece = (tap, k, group of 8 ci) of
  // w[cr0 + k][tap][co0 + 8 grp], byte offsets without the chunk's
  uint32_t woff[kDgNW];
#pragma unroll
  for (int i = 0; i < kDgNW; ++i) {
    const int p = tid + i * kDgThreads;
    const int pc = p < kDgWPieces ? p : kDgWPieces - 1;
    const int tap = pc >> 7, k = (pc >> 3) & 15, grp = pc & 7;
    woff[i] = (uint32_t)((k * 9 + tap) * g.Co + co0 + grp * 8) * 2u;
  }
  // load-side tile state: byte offsets of this thread's halo pieces (without the chunk's
  // channel offset) and their validity, once per tile
  int ld_tile = -1;
  uint32_t xoff[NX];
  uint32_t xok = 0u;
  auto load_geom = [&](int tile) {
    int q0, v0;
    tile_org(tile, &q0, &v0);
    xok = 0u;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int p = tid + i * kDgThreads;
      const int pc = p < xpieces ? p : xpieces - 1;
      const int e = pc >> 1, h = pc & 1;
      const int vr = e / WP, c = e - vr * WP;
      const int v = v0 + vr;
      const int n = v / HP, a = v - n * HP;
      const bool ok = p < xpieces && n < g.N && a < g.OH && c < g.OW;
      const int nc = n < g.N ? n : g.N - 1;
      const int ac = a < g.OH ? a : g.OH - 1, cc = c < g.OW ? c : g.OW - 1;
      xoff[i] = (uint32_t)(((nc * g.OH + ac) * g.OW + cc) * g.Cr + h * 8) * 2u;
      xok |= ok ? (1u << i) : 0u;
    }
  };
  auto load = [&](DgSet<NX>& st, int stage) {
    int cc;
    const int tile = tile_of(stage, &cc);
    if (tile != ld_tile) {  // uniform: the stage stream crossed into a new tile
      load_geom(tile);
      ld_tile = tile;
    }
    const uint32_t cr0b = (uint32_t)(cc * kDgKC) * 2u;
    const uint32_t wstepb = cr0b * 9u * (uint32_t)g.Co;
    st.ok = xok;
    const char* xc = reinterpret_cast<const char*>(dy);
    const char* wc = reinterpret_cast<const char*>(w);
#pragma unroll
    for (int i = 0; i < NX; ++i) st.x[i] = *reinterpret_cast<const u32x4*>(xc + (xoff[i] + cr0b));
#pragma unroll
    for (int i = 0; i < kDgNW; ++i) st.w[i] = *reinterpret_cast<const u32x4*>(wc + (woff[i] + wstepb));
  };
  auto store = [&](const DgSet<NX>& st, int buf) {
    __bf16* X = lds + buf * BE;
    __bf16* Wt = X + XE;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NX; ++i) {  // p >= xpieces: an entry past the image, never read
      const int p = tid + i * kDgThreads;
      *reinterpret_cast<u32x4*>(X + (p >> 1) * kDgRow + (p & 1) * 8) = (st.ok >> i) & 1u ? st.x[i] : z;
    }
#pragma unroll
    for (int i = 0; i < kDgNW; ++i) {
      const int p = tid + i * kDgThreads;  // pieces past 9 taps land in unused rows
      *reinterpret_cast<u32x4*>(Wt + (p >> 3) * kDgFRow + (p & 7) * 8) = st.w[i];
    }
  };

  const int kg = (lane >> 5) * 8;  // k-group: channels 8 (lane / 32) .. + 7 of the chunk
  // transposed-read roles (A operand): group gq of 16 lanes, lane 4q+p -> row q, channels 4p..4p+3
  const int gq = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int cho = 16 * (gq & 1) + 4 * p4, rwo = 8 * (gq >> 1) + q4;
  int bpos[JB];       // this lane's quad of block j as an LDS element offset of fragment A
  uint32_t dpos[JB];  // ... as a dx element offset of its pixel (2 a, 2 b), channel 0
  uint32_t dok[JB];   // bit 0: the quad is the tile's; bit 1: 2 a + 1 < H; bit 2: 2 b + 1 < W
  auto set_tile = [&](int tile) {
    int q0, q_end, v0;
    tile_org(tile, &q0, &v0, &q_end);
#pragma unroll
    for (int j = 0; j < JB; ++j) {
      int q = q0 + wave * (32 * JB) + j * 32 + (lane & 31);
      const bool in = q < q_end;
      if (!in) q = q_end - 1;  // past the tile: a duplicate, never stored
      const int n = q / ohw, rem = q - n * ohw;
      const int a = rem / g.OW, b = rem - a * g.OW;
      bpos[j] = (n * HP + a - v0) * RS + b * kDgRow + kg;
      dpos[j] = (uint32_t)((n * g.H + 2 * a) * g.W + 2 * b) * (uint32_t)g.Co;
      dok[j] = in ? (1u | (2 * a + 1 < g.H ? 2u : 0u) | (2 * b + 1 < g.W ? 4u : 0u)) : 0u;
    }
  };

  f32x16 acc[4][2][JB];  // [parity class][channel block][quad block]
  auto zero = [&]() {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
          for (int k = 0; k < 16; ++k) acc[c][i][j][k] = 0.f;
  };

  // a chunk's four B fragments per quad block are read once; tap t + 1's A fragments are
  // read while tap t's MFMAs run (one wave per SIMD: nothing else hides the LDS latency)
  auto fetch_a = [&](const __bf16* Wt, int tap, bf16x8 (&fa)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const __bf16* pa = Wt + (tap * 16 + rwo) * kDgFRow + i * 32 + cho;
      fa[i] = __builtin_shufflevector(tr4(pa), tr4(pa + 4 * kDgFRow), 0, 1, 2, 3, 4, 5, 6, 7);
    }
  };
  auto compute = [&](int buf) {
    const __bf16* X = lds + buf * BE;
    const __bf16* Wt = X + XE;
    bf16x8 fb[4][JB], fa[2][2];
#pragma unroll
    for (int f = 0; f < 4; ++f)  // A, B, C, D = dy(a + f / 2, b + f % 2)
#pragma unroll
      for (int j = 0; j < JB; ++j)
        fb[f][j] = *reinterpret_cast<const bf16x8*>(X + bpos[j] + (f >> 1) * RS + (f & 1) * kDgRow);
    fetch_a(Wt, 0, fa[0]);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int cur = tap & 1;
      const int r = tap / 3, s = tap - (tap / 3) * 3;
      const int cls = (r != 1 ? 2 : 0) + (s != 1 ? 1 : 0), f = (r == 0 ? 2 : 0) + (s == 0 ? 1 : 0);
      if (tap + 1 < 9) fetch_a(Wt, tap + 1, fa[cur ^ 1]);
      __builtin_amdgcn_sched_barrier(0);  // keep the reads ahead of this tap's MFMAs
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < JB; ++j)
          acc[cls][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[cur][i], fb[f][j], acc[cls][i][j], 0, 0, 0);
    }
  };

  // D[ci][quad]: lane -> quad (lane & 31) of block j; accumulator k -> channel
  // (k & 3) + 8 (k >> 2) + 4 (lane >> 5) of block i.  Class c = 2 dr + dc is pixel
  // (2 a + dr, 2 b + dc) of the quad
  auto epilogue = [&]() {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int dr = c >> 1, dc = c & 1;
#pragma unroll
      for (int j = 0; j < JB; ++j) {
        // lanes l and l ^ 32 hold the same quad; a v_permlane32_swap per dword of each
        // channel-group pair gives lane half (lane >> 5) 8 consecutive channels: 16-byte stores
        const uint32_t need = 1u | (dr ? 2u : 0u) | (dc ? 4u : 0u);
        const bool ok = (dok[j] & need) == need;
        const uint32_t pix = ok ? dpos[j] + (uint32_t)(dr * g.W + dc) * (uint32_t)g.Co : 0u;
        uint16_t* yo = dx + pix + co0 + 8 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          uint32_t v[4][2];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            bf16x4 b;
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = (__bf16)acc[c][i][j][4 * q + e];
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
      }
    }
  };

  // stage k of the stream: global -> register set k % DEPTH -> LDS buffer k & 1
  // (conv3x3s2.hip's pipeline: set (it + 1) % DEPTH goes to the buffer the previous
  // iteration finished reading and is reloaded with stage it + 1 + DEPTH)
  auto step = [&](int it, int buf, DgSet<NX>& nxt) {
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
    if (cc == nchunks - 1) epilogue();
  };
  DgSet<NX> sets[DEPTH];
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
}

}  // namespace

Conv3x3S2DgradGeom conv3x3s2_dgrad_geom(int64_t N, int64_t H, int64_t W, int64_t Cr, int64_t Co) {
  if (!conv3x3_args_ok(N, H, W, Cr, Co)) return Conv3x3S2DgradGeom{};
  Conv3x3S2DgradGeom g{(int)N, (int)H, (int)W, (int)Cr, (int)Co, (int)((H - 1) / 2 + 1), (int)((W - 1) / 2 + 1), 0, 0};
  g.wpb = conv3x3_wpb(g.N, g.OH, g.OW, g.Co);
  // stride key 3: the stride-2 INPUT GRADIENT's walk (1 and 2 are the forwards')
  g.vrows = conv3x3_cached_vrows(3, g.N, g.H, g.W, kDgTQ, g.wpb, [&g] { return conv3x3s2_dgrad_vrows(g); });
  return g;
}

int conv3x3s2_dgrad_vrows(const Conv3x3S2DgradGeom& g) {
  // the most virtual halo rows any tile of the partition touches; stops early once the
  // halo cannot fit (the answer is then only "too many")
  const int64_t Q = (int64_t)g.N * g.OH * g.OW;
  const int ohw = g.OH * g.OW, HP = g.OH + 1, WP = g.OW + 1;
  const int cap = kDgNX * kDgThreads / 2 / WP;  // rows the halo buffer holds
  int best = 0;
  for (int j = 0; j < g.wpb && best <= cap; ++j) {
    const int64_t lo = Q * j / g.wpb, hi = Q * (j + 1) / g.wpb;
    for (int64_t q0 = lo; q0 < hi && best <= cap; q0 += kDgTQ) {
      const int64_t q1 = (q0 + kDgTQ < hi ? q0 + kDgTQ : hi) - 1;
      const int n0 = (int)(q0 / ohw), a0 = (int)((q0 % ohw) / g.OW);
      const int n1 = (int)(q1 / ohw), a1 = (int)((q1 % ohw) / g.OW);
      const int rows = (n1 * HP + a1 + 1) - (n0 * HP + a0) + 1;
      if (rows > best) best = rows;
    }
  }
  return best;
}

int conv3x3s2_dgrad_pieces_per_thread(const Conv3x3S2DgradGeom& g) {
  return (int)(((int64_t)g.vrows * (g.OW + 1) * 2 + kDgThreads - 1) / kDgThreads);
}

int conv3x3s2_dgrad_tq() { return kDgTQ; }
int conv3x3s2_dgrad_nx(const Conv3x3S2DgradGeom& g) {
  // the instance: halo pieces per thread it loads and stores every chunk (ResNet's shapes need 2)
  const int pieces = conv3x3s2_dgrad_pieces_per_thread(g);
  return pieces <= 2 ? 2 : (pieces >= kDgNX ? kDgNX : pieces);
}

bool conv3x3s2_dgrad_ok(const Conv3x3S2DgradGeom& g) {
  // 32-bit byte offsets into dy and w, 32-bit element offsets into dx, 32-bit virtual rows;
  // the halo of every tile fits the buffer
  return g.N > 0 && g.H > 0 && g.W > 0 && g.Cr > 0 && g.Co > 0 && g.Cr % kDgKC == 0 && g.Co % kDgTN == 0 &&
         g.OH == (g.H - 1) / 2 + 1 && g.OW == (g.W - 1) / 2 + 1 && g.vrows > 0 && g.wpb > 0 &&
         g.wpb <= (int64_t)g.N * g.OH * g.OW &&
         (int64_t)g.vrows * (g.OW + 1) <= kDgNX * kDgThreads / 2 &&
         (int64_t)g.N * (g.OH + 1) < (1ll << 30) &&
         (int64_t)g.N * g.OH * g.OW * g.Cr < (1ll << 31) && (int64_t)g.N * g.H * g.W * g.Co < (1ll << 31) &&
         (int64_t)g.Cr * 9 * g.Co < (1ll << 31);
}

bool launch_conv3x3s2_dgrad(const uint16_t* dy, const uint16_t* w, uint16_t* dx, const Conv3x3S2DgradGeom& g,
                            hipStream_t st) {
  if (!conv3x3s2_dgrad_ok(g)) return false;
  // persistent: one workgroup per (quad range, dx-channel block)
  const dim3 grid((unsigned)(g.wpb * (g.Co / kDgTN)));
  switch (conv3x3s2_dgrad_nx(g)) {
    case 2:
      hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<2>, grid, dim3(kDgThreads), 0, st, dy, w, dx, g);
      break;
    case 3:
      hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<3>, grid, dim3(kDgThreads), 0, st, dy, w, dx, g);
      break;
    default:
      hipLaunchKernelGGL(conv3x3s2_dgrad_kernel<4>, grid, dim3(kDgThreads), 0, st, dy, w, dx, g);
      break;
  }
  return true;
}

}  // namespace rla
