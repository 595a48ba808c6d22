// General-width training step and forward of the MNIST classifier MLP (784 -> L1 -> L2 -> 10)
// for gfx950: every 1 <= L1, L2 <= 512 but the odd multiples of 16 (kernels.h), 1 <= B <= 4096
// (the forward: any B).  The
// table kernels hold whole layers per CU (mlp_step3.hip) or alias H1 / H2 / Z / dZ into the dead
// X image of a slab with whole-K accumulators for every column tile of layer 1
// (mlp_step_wide.hip, L1 <= 128, L2 <= 256); neither plan reaches 512.  Here the work is split
// over columns as well as rows, the widths are run-time values (ONE instance of each kernel, the
// block shapes compile-time constants, the grid sized at run time), and the contract is
// mlp_train_step's as the wide step honours it.  Four launches, every reduction in a fixed order
// (no float atomics in the step), so two runs from one state -- eager or replayed from a captured
// graph -- agree bit for bit.
//
//   1. layer 1  grid (64-row slab) x (64-column block of L1), 512 threads.  Each workgroup
//               stages its slab's pixels as bf16 into the padded LDS image (64 x 808, rows 20
//               dwords apart: conflict-free 16-byte reads) and runs v_mfma_f32_16x16x32_bf16
//               over K = 784: wave w owns row tile w & 3 and the column tiles (w >> 2) and
//               (w >> 2) + 2 of the block, fp32 accumulators, W1 streamed from the fp32 master
//               in 32-wide K chunks and rounded to bf16 where it is staged.  relu(. + b1) leaves
//               twice: row-major H1 [Bp][L1] for the head, transposed H1T [L1][Bp] for dW2.
//               Column block 0 also parks XT.  A column tile at or past L1 (the last block of
//               L1 = 96, 160, ...) multiplies zero weights and stores nothing.  A batch-32,
//               L1 = 512 step thus streams W1 through 8 CUs, not one.
//   2. head     one 512-thread workgroup per slab.  H1 comes from HBM into LDS (stride L1 + 8),
//               layer 2 runs one 16-column tile of L2 per wave at a time against all four row
//               tiles (one W2 fragment, four MFMAs), then layer 3, softmax / NLL / accuracy and
//               dZ as in the wide step; dH2 overwrites H2 in LDS -- the lane that reads an
//               element's ReLU mask is the lane that overwrites it -- and dH1 is formed from it.
//               LDS at 512/512: 2 x 66,560 B (H1, H2) + Z 4,096 + dZ 5,120 + labels 256 =
//               142,592 B of the 160 KB; the 512 cap comes from it.  The block is declared at
//               that size whatever the widths: one workgroup per slab and CU anyway.
//               Parked: H2T, dH2T, dZT, dH1T and the slab's (sum NLL, #correct, #rows).
//               The forward-only instance (TRAIN = false) stops after the softmax and writes
//               mlp_eval's outputs: two 32-row chunks per slab, or one atomic pair.
//   3. param    one wave per 16x16 gradient tile and batch slice over the parked [feature][Bp]
//               rows: mlp_wide_param_kernel's scheme with run-time widths; same slice rule.
//   4. apply    mlp_apply.h, the wide step's own last launch.
//
// Where this leaves the starting design: dH1 is NOT written back over H1 in LDS -- nothing reads
// it there; it goes from the accumulators straight to dH1T, masked by the H1 element the same
// lane reads.  Layer 2 / dH2 / dH1 give a wave one column tile and all four row tiles (not one
// (row, column) tile as the wide slab does): the W2 / W3 fragment, which dH1 gathers with a
// stride of L1 floats, is fetched once for four MFMAs.
//
// Ragged widths (L1 or L2 no multiple of 32) run instances of their own (RAGGED = true); the
// multiples of 32 keep the instances they had.  Padded compute, true storage: with L1p, L2p the
// widths rounded up to 32, everything the MFMA core touches -- the LDS images of H1 / H2, the
// parked [feature][Bp] operands, the h1 hand-off, the tile lists -- keeps the padded extents,
// so no tile loop, LDS stride or workspace offset changes shape; the parameter, gradient and
// Adam arenas keep the true widths (goff), and nothing keeps a padded copy of the weights.
//   * zero-fill, never over-read: a weight fragment's elements at or past the row's end (K pad)
//     and whole rows at or past the width (column pad) are exact zeros in the registers (ldw8),
//     padded bias lanes read 0, so the padded columns of H1 / H2 are relu(0 + 0) = 0 and stay 0
//     through dH2 / dH1 (their ReLU mask).  What lies behind a row in the arena -- the next
//     row's first weight, b2 behind W2 -- is never loaded, so an Inf there cannot meet a 0.
//   * alignment: with L1 % 4 != 0 the tensors' offsets and the W2 / W3 row starts are only
//     4-byte aligned.  ldw8 loads dwords there and float4s where a lane's eight floats exist
//     and start a 16-byte line.  W1's rows are 784 floats: its stream stays float4, only the
//     row count is masked.
//   * masked stores: launch 3 computes whole 16x16 tiles over the padded extents and stores the
//     elements inside the true tensors only.
//   * the sums: a ragged step adds the same numbers in the same order as the aligned step at
//     (L1p, L2p) on zero-padded parameters, plus exact zeros -- the two agree bit for bit.
// The arena may pack the six tensors back to back or each on a multiple of 4 floats (goff's al).
//
// Launches 1 and 2 only READ counters and launch 4 is the only writer; block (0, 0) of launch 1
// leaves (t, cursor, rows) in the workspace header for launch 4.
#include "common.h"
#include "kernels.h"
#include "mlp_apply.h"
#include "mlp_common.h"

namespace rla {
namespace {

using namespace mlp;

constexpr int kBC = 64;          // rows per slab
constexpr int kXS = 808;         // LDS row stride of X (bf16)
constexpr int kKS1 = 25;         // ceil(784 / 32) K steps of layer 1
constexpr int kThreads = 512;    // launches 1 and 2: 8 waves
constexpr int kWaves = kThreads / 64;
constexpr int kMT = kBC / 16;    // 16-row tiles per slab
constexpr int kDZS = 40;         // LDS row stride of dZ (K padded to 32 + 8)
constexpr int kPThreads = 256;   // param launch
constexpr int kCB = kMLPGeneralColBlock;
constexpr int kMaxW = kMLPGeneralMaxWidth;
constexpr size_t kHeadLds = 2 * (size_t)kBC * (kMaxW + 8) * 2 + kBC * 16 * 4 + kBC * kDZS * 2 + kBC * 4;
static_assert(kHeadLds <= 160 * 1024 - 1024, "the head's LDS plan");
static_assert(kCB == 64 && kWaves == 8, "a wave owns one row tile and two of the block's four column tiles");

// the arena with run-time widths (mlp_common.h Off)
struct GOff {
  int64_t W1, B1, W2, B2, W3, B3, NP;
};
// al = 1: the six tensors back to back; al = 4: each starts on a multiple of 4 floats, as a
// parameter arena with 16-byte aligned views packs them (the two agree where L1 and L2 are
// multiples of 4).  NP ends with b3: no pad behind the last tensor.
inline __host__ __device__ GOff goff(int L1, int L2) {
  GOff o;
  o.W1 = 0; o.B1 = (int64_t)L1 * kD; o.W2 = o.B1 + L1; o.B2 = o.W2 + (int64_t)L2 * L1;
  o.W3 = o.B2 + L2; o.B3 = o.W3 + kNC * L2; o.NP = o.B3 + kNC;
  return o;
}
inline __host__ __device__ GOff goff(int L1, int L2, int al) {
  GOff o;
  o.W1 = 0; o.B1 = (int64_t)L1 * kD;
  o.W2 = (o.B1 + L1 + al - 1) / al * al;
  o.B2 = (o.W2 + (int64_t)L2 * L1 + al - 1) / al * al;
  o.W3 = (o.B2 + L2 + al - 1) / al * al;
  o.B3 = (o.W3 + kNC * L2 + al - 1) / al * al;
  o.NP = o.B3 + kNC;
  return o;
}

// Ragged widths: what the MFMA core touches (LDS images, parked operands, the h1 hand-off, the
// tile lists) keeps the extent rounded up to 32; the arenas keep the true one.
inline __host__ __device__ int pad32(int w) { return (w + 31) & ~31; }

// Parked operands (element offsets): the wide step's six, [feature][Bp] each, then H1 [Bp][L1].
struct GPark {
  int64_t xt, h1t, h2t, dh2t, dzt, dh1t, h1, total;
};
inline __host__ __device__ GPark gpark(int L1, int L2, int64_t Bp) {
  GPark p;
  p.xt = 0;
  p.h1t = p.xt + kD * Bp;
  p.h2t = p.h1t + L1 * Bp;
  p.dh2t = p.h2t + L2 * Bp;
  p.dzt = p.dh2t + L2 * Bp;
  p.dh1t = p.dzt + 16 * Bp;
  p.h1 = p.dh1t + L1 * Bp;
  p.total = p.h1 + L1 * Bp;
  return p;
}

inline __host__ __device__ int gtasks(int L1, int L2) {
  return kTiles * (L1 / 16) + (L2 / 16) * (L1 / 16) + L2 / 16 + L1 / 16 + L2 / 16 + 1;
}

// What launches 1 and 2 read, for the step and for the forward alike.
struct GenArgs {
  const uint8_t* x_u8;
  const float* x_f32;
  const int64_t* labels;
  const int64_t* order;     // step: the epoch's order (u8 mode); forward: index[B]
  const int64_t* counters;  // step: device state; forward: null (cursor 0, every row of B)
  int64_t n_batches;
  int B, last_rows, L1, L2;
  float x_scale, x_shift;
  const float* params;
  __bf16* h1;               // [Bp][L1]
  __bf16* park;             // step: the parked operands; forward: null
  int64_t Bp;
  int64_t* hdr;             // step only
  float* slab_stats;        // step only
  float* logits;            // forward only, optional
  float* out;               // forward only
  int partials;
  int align;                // ragged instances only: goff's al (the others never read it)
};

__device__ __forceinline__ void st4(__bf16* p, bf16x4 v) { *reinterpret_cast<bf16x4*>(p) = v; }

// Ragged rows: p[0 .. 8) as bf16 with every element at or past nv an exact zero -- never what
// lies behind the row in the arena (the next row's first weight, or the next tensor).  p needs
// 4-byte alignment only; a lane whose eight floats exist and start a 16-byte line takes two
// float4 loads (every lane of an interior K step when L1 is a multiple of 4).
__device__ __forceinline__ bf16x8 ldw8(const float* p, int nv) {
  if (nv >= 8 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return cvt8(ld4(p), ld4(p + 4));
  bf16x8 v = zero8();
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < nv) v[j] = (__bf16)p[j];
  return v;
}

// batch position and size from the device state (a captured graph replays at any cursor)
__device__ __forceinline__ void batch_of(const GenArgs& a, bool u8, int64_t& cursor, int& rows) {
  cursor = (u8 && a.counters) ? a.counters[1] : 0;
  rows = (u8 && a.counters && cursor == a.n_batches - 1) ? a.last_rows : a.B;
}

// ---------------------------------------------------------------------------------------
// Launch 1: layer 1 of one (slab, column block).
// ---------------------------------------------------------------------------------------
template <bool U8, bool RAGGED>
__global__ __launch_bounds__(kThreads) void mlp_general_l1_kernel(GenArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 sX[kBC * kXS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int slab = blockIdx.x, cb = blockIdx.y, row0 = slab * kBC;
  const int L1 = a.L1;
  const int L1p = RAGGED ? pad32(L1) : L1;  // columns of H1 / H1T: those in [L1, L1p) are stored as zeros
  const int64_t Bp = a.Bp;
  int64_t cursor;
  int rows;
  batch_of(a, U8, cursor, rows);
  const int nvalid = min(kBC, max(0, rows - row0));
  const int64_t* idx = U8 ? a.order + cursor * a.B : nullptr;
  if (a.hdr && slab == 0 && cb == 0 && tid == 0) {
    a.hdr[0] = (a.counters ? a.counters[0] : 0) + 1;
    a.hdr[1] = cursor;
    a.hdr[2] = rows;
  }

  // ---- stage the slab's rows as bf16 (rows past the batch: zero pixels) ----
  if constexpr (U8) {
    constexpr int CPR = kD / 16;
    for (int t = tid; t < kBC * CPR; t += kThreads) {
      const int r = t / CPR, cc = t - r * CPR;
      bf16x8 lo = zero8(), hi = zero8();
      if (r < nvalid) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.x_u8 + idx[row0 + r] * kD + cc * 16);
        u8x16_to_bf16(v, lo, hi, a.x_scale, a.x_shift);
      }
      __bf16* dst = sX + r * kXS + cc * 16;
      *reinterpret_cast<bf16x8*>(dst) = lo;
      *reinterpret_cast<bf16x8*>(dst + 8) = hi;
    }
  } else {
    constexpr int CPR = kD / 8;
    for (int t = tid; t < kBC * CPR; t += kThreads) {
      const int r = t / CPR, cc = t - r * CPR;
      bf16x8 v = zero8();
      if (r < nvalid) {
        const float* src = a.x_f32 + (int64_t)(row0 + r) * kD + cc * 8;
        v = cvt8(ld4(src), ld4(src + 4));
      }
      *reinterpret_cast<bf16x8*>(sX + r * kXS + cc * 8) = v;
    }
  }
  for (int t = tid; t < kBC * 3; t += kThreads) {
    const int r = t / 3, j = t - r * 3;
    *reinterpret_cast<bf16x8*>(sX + r * kXS + kD + j * 8) = zero8();
  }
  __syncthreads();

  // ---- column block 0 parks X^T: 8 consecutive rows of one pixel per 16-byte store ----
  if (a.park && cb == 0) {
    __bf16* xt = a.park;  // GPark::xt == 0
    for (int t = tid; t < kD * (kBC / 8); t += kThreads) {
      const int c = t & 7, pix = t >> 3;
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = sX[(c * 8 + j) * kXS + pix];
      *reinterpret_cast<bf16x8*>(xt + (int64_t)pix * Bp + row0 + c * 8) = v;
    }
  }

  // ---- wave wv: row tile wv & 3, column tiles (wv >> 2) and (wv >> 2) + 2 of the block ----
  const float* W1 = a.params;
  const float* b1 = a.params + (int64_t)L1 * kD;
  const int mt1 = wv & 3, ct0 = wv >> 2;
  const int nc0 = cb * kCB + ct0 * 16, nc1 = nc0 + 32;  // first column of each tile
  const bool live0 = nc0 < L1p, live1 = nc1 < L1p;      // wave-uniform: L1p is a multiple of 16
  // ragged: whether this lane's W1 row exists (a row at or past L1 is a fragment of zeros: the
  // row count is ragged, the 784-float rows themselves stay 16-byte aligned float4 streams)
  const bool ok0 = !RAGGED || nc0 + r16 < L1, ok1 = !RAGGED || nc1 + r16 < L1;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const float* w0 = W1 + (int64_t)(RAGGED ? (ok0 ? nc0 + r16 : 0) : (live0 ? nc0 : 0) + r16) * kD;
  const float* w1 = W1 + (int64_t)(RAGGED ? (ok1 ? nc1 + r16 : 0) : (live1 ? nc1 : 0) + r16) * kD;
#pragma unroll 5
  for (int ks = 0; ks < kKS1; ++ks) {
    const int k = ks * 32 + 8 * g;
    const bf16x8 afrag = ld8(sX + (mt1 * 16 + r16) * kXS + k);
    bf16x8 f0 = zero8(), f1 = zero8();
    if (k < kD) {
      if (live0 && ok0) f0 = cvt8(ld4(w0 + k), ld4(w0 + k + 4));
      if (live1 && ok1) f1 = cvt8(ld4(w1 + k), ld4(w1 + k + 4));
    }
    acc0 = mfma16(afrag, f0, acc0);
    acc1 = mfma16(afrag, f1, acc1);
  }
  __bf16* h1t = a.park ? a.park + gpark(L1p, a.L2, Bp).h1t : nullptr;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!(j ? live1 : live0)) continue;
    const f32x4 acc = j ? acc1 : acc0;
    const int n = (j ? nc1 : nc0) + r16;
    const float bias = (j ? ok1 : ok0) ? b1[n] : 0.f;  // a padded column: relu(0 + 0)
    bf16x4 t4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __bf16 h = (__bf16)fmaxf(acc[i] + bias, 0.f);
      a.h1[(int64_t)(row0 + mt1 * 16 + 4 * g + i) * L1p + n] = h;
      t4[i] = h;
    }
    if (h1t) st4(h1t + (int64_t)n * Bp + row0 + mt1 * 16 + 4 * g, t4);
  }
}

// ---------------------------------------------------------------------------------------
// Launch 2: the head of one slab.
// ---------------------------------------------------------------------------------------
template <bool TRAIN, bool U8, bool RAGGED>
__global__ __launch_bounds__(kThreads) void mlp_general_head_kernel(GenArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kHeadLds];
  const int L1 = a.L1, L2 = a.L2;
  const int L1p = RAGGED ? pad32(L1) : L1, L2p = RAGGED ? pad32(L2) : L2;
  const int H1S = L1p + 8, H2S = L2p + 8, TN1 = L1p / 16, TN2 = L2p / 16;
  __bf16* sH1 = (__bf16*)smem;
  __bf16* sH2 = sH1 + kBC * H1S;
  float* sZ = (float*)(sH2 + kBC * H2S);
  __bf16* sdZ = (__bf16*)(sZ + kBC * 16);
  int* sY = (int*)(sdZ + kBC * kDZS);

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int slab = blockIdx.x, row0 = slab * kBC;
  const int64_t Bp = a.Bp;
  const GPark pk = gpark(L1p, L2p, Bp);
  const GOff o = RAGGED ? goff(L1, L2, a.align) : goff(L1, L2);
  int64_t cursor;
  int rows;
  batch_of(a, U8, cursor, rows);
  const int nvalid = min(kBC, max(0, rows - row0));
  const int64_t* idx = U8 ? a.order + cursor * a.B : nullptr;
  const float* W2 = a.params + o.W2;
  const float* b2 = a.params + o.B2;
  const float* W3 = a.params + o.W3;
  const float* b3 = a.params + o.B3;

  // ---- the slab's H1 rows into LDS, its labels (rows past the batch: -1) ----
  const int cpr = L1p / 8;
  for (int t = tid; t < kBC * cpr; t += kThreads) {
    const int r = t / cpr, c = t - r * cpr;
    *reinterpret_cast<bf16x8*>(sH1 + r * H1S + c * 8) = ld8(a.h1 + (int64_t)(row0 + r) * L1p + c * 8);
  }
  if (tid < kBC) {
    int y = -1;
    if (tid < nvalid) y = (int)(U8 ? a.labels[idx[row0 + tid]] : a.labels[row0 + tid]);
    sY[tid] = y;
  }
  __syncthreads();

  // ---- layer 2: a wave takes column tile nt against the four row tiles ----
  for (int nt = wv; nt < TN2; nt += kWaves) {
    f32x4 acc[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int n = nt * 16 + r16;
    const bool nok = !RAGGED || n < L2;  // ragged: a column at or past L2 has zero weights and a zero bias
    const float* wrow = W2 + (int64_t)(nok ? n : 0) * L1;
    for (int ks = 0; ks < L1p / 32; ++ks) {
      const int k = ks * 32 + 8 * g;
      bf16x8 bfrag;
      if constexpr (RAGGED) bfrag = ldw8(wrow + k, nok ? L1 - k : 0);
      else bfrag = cvt8(ld4(wrow + k), ld4(wrow + k + 4));
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt) acc[mt] = mfma16(ld8(sH1 + (mt * 16 + r16) * H1S + k), bfrag, acc[mt]);
    }
    const float bias = nok ? b2[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
      bf16x4 t4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const __bf16 h = (__bf16)fmaxf(acc[mt][i] + bias, 0.f);
        sH2[(mt * 16 + 4 * g + i) * H2S + n] = h;
        t4[i] = h;
      }
      if constexpr (TRAIN) st4(a.park + pk.h2t + (int64_t)n * Bp + row0 + mt * 16 + 4 * g, t4);
    }
  }
  __syncthreads();

  // ---- layer 3 (classes padded to 16): waves 0..3, one row tile each ----
  if (wv < kMT) {
    const int mt = wv;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < L2p / 32; ++ks) {
      const int k = ks * 32 + 8 * g;
      bf16x8 bfrag = zero8();
      if constexpr (RAGGED) {
        if (r16 < kNC) bfrag = ldw8(W3 + r16 * L2 + k, L2 - k);
      } else {
        if (r16 < kNC) bfrag = cvt8(ld4(W3 + r16 * L2 + k), ld4(W3 + r16 * L2 + k + 4));
      }
      acc = mfma16(ld8(sH2 + (mt * 16 + r16) * H2S + k), bfrag, acc);
    }
    if (r16 < kNC) {
      const float bias = b3[r16];
#pragma unroll
      for (int i = 0; i < 4; ++i) sZ[(mt * 16 + 4 * g + i) * 16 + r16] = acc[i] + bias;
    }
  }
  __syncthreads();

  // ---- log-softmax / NLL / accuracy (/ dZ): wave 0, one lane per row ----
  if (wv == 0) {
    const int r = lane, y = sY[r];
    const float inv_rows = 1.f / (float)rows;
    float loss = 0.f, hit = 0.f, cnt = 0.f;
    bf16x8 d8[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) d8[q] = zero8();
    if (y >= 0) {
      float z[kNC], m = -INFINITY;
      int arg = 0;
#pragma unroll
      for (int j = 0; j < kNC; ++j) {
        z[j] = sZ[r * 16 + j];
        if (z[j] > m) { m = z[j]; arg = j; }
      }
      float p[kNC], sum = 0.f;
#pragma unroll
      for (int j = 0; j < kNC; ++j) { p[j] = expf(z[j] - m); sum += p[j]; }
      const float inv = 1.f / sum;
      const float lse = m + logf(sum);
      loss = lse - z[y];
      hit = (arg == y) ? 1.f : 0.f;
      cnt = 1.f;
      if constexpr (TRAIN) {
#pragma unroll
        for (int j = 0; j < kNC; ++j) d8[j >> 3][j & 7] = (__bf16)((p[j] * inv - (j == y ? 1.f : 0.f)) * inv_rows);
      } else if (a.logits) {
#pragma unroll
        for (int j = 0; j < kNC; ++j) a.logits[(int64_t)(row0 + r) * kNC + j] = z[j] - lse;
      }
    }
    if constexpr (TRAIN) {
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x8*>(sdZ + r * kDZS + 8 * q) = d8[q];
#pragma unroll
      for (int j = 0; j < 16; ++j) a.park[pk.dzt + (int64_t)j * Bp + row0 + r] = d8[j >> 3][j & 7];
      // fixed butterfly: the same tree in every run
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        loss += __shfl_down(loss, off, 64);
        hit += __shfl_down(hit, off, 64);
        cnt += __shfl_down(cnt, off, 64);
      }
      if (lane == 0) {
        float* st = a.slab_stats + slab * 4;
        st[0] = loss; st[1] = hit; st[2] = cnt; st[3] = 0.f;
      }
    } else {
      // lanes 0 and 32 end with the sums of the slab's two 32-row chunks
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        loss += __shfl_down(loss, off, 64);
        hit += __shfl_down(hit, off, 64);
      }
      if (a.partials) {
        const int c = slab * 2 + (lane >> 5);
        if ((lane & 31) == 0 && c < (a.B + 31) / 32) {
          a.out[2 * c] = loss;
          a.out[2 * c + 1] = hit;
        }
      } else {
        loss += __shfl_down(loss, 32, 64);
        hit += __shfl_down(hit, 32, 64);
        if (lane == 0) {
          atomicAdd(&a.out[0], loss);
          atomicAdd(&a.out[1], hit);
        }
      }
    }
  }
  if constexpr (TRAIN) {
    __syncthreads();

    // ---- dH2 = (dZ W3) * (H2 > 0): in place of H2, and parked transposed ----
    for (int nt = wv; nt < TN2; nt += kWaves) {
      const int n = nt * 16 + r16;
      bf16x8 bfrag = zero8();
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = 8 * g + jj;
        if (j < kNC && (!RAGGED || n < L2)) bfrag[jj] = (__bf16)W3[j * L2 + n];
      }
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt) {
        const bf16x8 afrag = ld8(sdZ + (mt * 16 + r16) * kDZS + 8 * g);
        const f32x4 acc = mfma16(afrag, bfrag, f32x4{0.f, 0.f, 0.f, 0.f});
        bf16x4 t4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          __bf16* hp = sH2 + (mt * 16 + 4 * g + i) * H2S + n;
          const __bf16 d = ((float)(*hp) > 0.f) ? (__bf16)acc[i] : (__bf16)0.f;
          *hp = d;
          t4[i] = d;
        }
        st4(a.park + pk.dh2t + (int64_t)n * Bp + row0 + mt * 16 + 4 * g, t4);
      }
    }
    __syncthreads();

    // ---- dH1 = (dH2 W2) * (H1 > 0), parked transposed ----
    for (int ct = wv; ct < TN1; ct += kWaves) {
      const int m = ct * 16 + r16;
      f32x4 acc[kMT];
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < L2p / 32; ++ks) {
        const int k = ks * 32 + 8 * g;
        bf16x8 bfrag;
        if constexpr (RAGGED) {
          bfrag = zero8();
#pragma unroll
          for (int jj = 0; jj < 8; ++jj)
            if (m < L1 && k + jj < L2) bfrag[jj] = (__bf16)W2[(int64_t)(k + jj) * L1 + m];
        } else {
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) bfrag[jj] = (__bf16)W2[(int64_t)(k + jj) * L1 + m];
        }
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) acc[mt] = mfma16(ld8(sH2 + (mt * 16 + r16) * H2S + k), bfrag, acc[mt]);
      }
#pragma unroll
      for (int mt = 0; mt < kMT; ++mt) {
        bf16x4 t4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const __bf16 hv = sH1[(mt * 16 + 4 * g + i) * H1S + m];
          t4[i] = ((float)hv > 0.f) ? (__bf16)acc[mt][i] : (__bf16)0.f;
        }
        st4(a.park + pk.dh1t + (int64_t)m * Bp + row0 + mt * 16 + 4 * g, t4);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Launch 3: one wave per (gradient tile, batch slice).  D[i][j] = sum_b A^T[i][b] B^T[j][b]
// over the slice's K steps; lane (r16, g) holds D[4 g + i][r16].
// ---------------------------------------------------------------------------------------
template <bool RAGGED>
__device__ __forceinline__ void param_tile(const MLPWideArgs w, int align) {
  const int L1 = w.step.L1, L2 = w.step.L2;
  const int L1p = RAGGED ? pad32(L1) : L1, L2p = RAGGED ? pad32(L2) : L2, TN1 = L1p / 16, TN2 = L2p / 16;
  const int NT_W1 = kTiles * TN1, NT_W2 = TN2 * TN1, NT_W3 = TN2, NT_B = TN1 + TN2 + 1;
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
  const int task = blockIdx.x * (kPThreads / 64) + (threadIdx.x >> 6);
  if (task >= NT_W1 + NT_W2 + NT_W3 + NT_B) return;  // whole waves; the kernel has no barrier
  const int s = blockIdx.y, S = gridDim.y;
  const int64_t Bp = w.Bp;
  const int nk = (int)(Bp / 32);
  const int ks0 = (int)((int64_t)s * nk / S), ks1 = (int)((int64_t)(s + 1) * nk / S);
  const GPark pk = gpark(L1p, L2p, Bp);
  const GOff o = RAGGED ? goff(L1, L2, align) : goff(L1, L2);
  const __bf16* park = reinterpret_cast<const __bf16*>(w.park);
  float* out = w.part + (int64_t)s * w.np_pad;

  const __bf16* arow;            // A^T row of this lane
  const __bf16* brow = nullptr;  // B^T row of this lane (null: a fragment of ones -- the bias sums)
  int kind, t0 = task, t1 = 0;
  if (task < NT_W1) {
    // dW1[m][pix] = sum_b X[b][pix] dH1[b][m]: rows pix (a float4 of the arena), columns m
    kind = 0; t0 = task % kTiles; t1 = task / kTiles;
    arow = park + pk.xt + (int64_t)(t0 * 16 + r16) * Bp;
    brow = park + pk.dh1t + (int64_t)(t1 * 16 + r16) * Bp;
  } else if (task < NT_W1 + NT_W2) {
    // dW2[n][m] = sum_b dH2[b][n] H1[b][m]
    kind = 1; t0 = (task - NT_W1) % TN2; t1 = (task - NT_W1) / TN2;
    arow = park + pk.dh2t + (int64_t)(t0 * 16 + r16) * Bp;
    brow = park + pk.h1t + (int64_t)(t1 * 16 + r16) * Bp;
  } else if (task < NT_W1 + NT_W2 + NT_W3) {
    // dW3[j][n] = sum_b dZ[b][j] H2[b][n]
    kind = 2; t0 = task - NT_W1 - NT_W2;
    arow = park + pk.dzt + (int64_t)r16 * Bp;
    brow = park + pk.h2t + (int64_t)(t0 * 16 + r16) * Bp;
  } else {
    // biases: row sums of dH1^T, dH2^T, dZ^T
    kind = 3; t0 = task - NT_W1 - NT_W2 - NT_W3;
    if (t0 < TN1) arow = park + pk.dh1t + (int64_t)(t0 * 16 + r16) * Bp;
    else if (t0 < TN1 + TN2) arow = park + pk.dh2t + (int64_t)((t0 - TN1) * 16 + r16) * Bp;
    else arow = park + pk.dzt + (int64_t)r16 * Bp;
  }
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int ks = ks0; ks < ks1; ++ks) {
    const int k = ks * 32 + 8 * g;
    const bf16x8 afrag = ld8(arow + k);
    const bf16x8 bfrag = brow ? ld8(brow + k) : ones;
    acc = mfma16(afrag, bfrag, acc);
  }
  // ragged: whole tiles were computed over the padded extents; only what lies inside the true
  // [L1][784], [L2][L1], [10][L2], [L1], [L2] is stored -- an edge tile's other elements would
  // land in the next row or the next tensor's gradient
  if (kind == 0) {
    if (!RAGGED || t1 * 16 + r16 < L1)
      *reinterpret_cast<F4*>(out + o.W1 + (int64_t)(t1 * 16 + r16) * kD + t0 * 16 + 4 * g) =
          F4{{acc[0], acc[1], acc[2], acc[3]}};
  } else if (kind == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (!RAGGED || (t0 * 16 + 4 * g + i < L2 && t1 * 16 + r16 < L1))
        out[o.W2 + (int64_t)(t0 * 16 + 4 * g + i) * L1 + t1 * 16 + r16] = acc[i];
  } else if (kind == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * g + i < kNC && (!RAGGED || t0 * 16 + r16 < L2)) out[o.W3 + (int64_t)(4 * g + i) * L2 + t0 * 16 + r16] = acc[i];
  } else if (r16 == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * g + i;
      if (t0 < TN1) {
        if (!RAGGED || t0 * 16 + e < L1) out[o.B1 + t0 * 16 + e] = acc[i];
      } else if (t0 < TN1 + TN2) {
        if (!RAGGED || (t0 - TN1) * 16 + e < L2) out[o.B2 + (t0 - TN1) * 16 + e] = acc[i];
      } else if (e < kNC) {
        out[o.B3 + e] = acc[i];
      }
    }
    if (RAGGED && g == 0 && t0 == TN1 + TN2) {
      // the words between the tensors of an aligned arena (up to 3 behind b1, W2, b2, W3; none
      // where align is 1): a zero gradient in every slice, whatever the workspace held before
      auto zero = [out](int64_t b, int64_t e) { for (; b < e; ++b) out[b] = 0.f; };
      zero(o.B1 + L1, o.W2);
      zero(o.W2 + (int64_t)L2 * L1, o.B2);
      zero(o.B2 + L2, o.W3);
      zero(o.W3 + (int64_t)kNC * L2, o.B3);
    }
  }
}

// The ragged instances where a width is no multiple of 32; the others run the instruction
// streams they always ran.  Layer 1 looks at L1 alone (96/40: its aligned instance, a ragged head).
// the aligned instance keeps its one argument (and with it its instruction stream)
__global__ __launch_bounds__(kPThreads) void mlp_general_param_kernel(MLPWideArgs w) { param_tile<false>(w, 1); }
__global__ __launch_bounds__(kPThreads) void mlp_general_param_ragged_kernel(MLPWideArgs w, int align) {
  param_tile<true>(w, align);
}

template <bool TRAIN, bool U8>
void launch_forward_u8(const GenArgs& g, int nslab, int ncb, hipStream_t stream) {
  if (g.L1 % 32) hipLaunchKernelGGL((mlp_general_l1_kernel<U8, true>), dim3(nslab, ncb), dim3(kThreads), 0, stream, g);
  else hipLaunchKernelGGL((mlp_general_l1_kernel<U8, false>), dim3(nslab, ncb), dim3(kThreads), 0, stream, g);
  if (g.L1 % 32 || g.L2 % 32)
    hipLaunchKernelGGL((mlp_general_head_kernel<TRAIN, U8, true>), dim3(nslab), dim3(kThreads), 0, stream, g);
  else hipLaunchKernelGGL((mlp_general_head_kernel<TRAIN, U8, false>), dim3(nslab), dim3(kThreads), 0, stream, g);
}

template <bool TRAIN>
void launch_forward(const GenArgs& g, int nslab, int ncb, hipStream_t stream) {
  if (g.x_u8) launch_forward_u8<TRAIN, true>(g, nslab, ncb, stream);
  else launch_forward_u8<TRAIN, false>(g, nslab, ncb, stream);
}

}  // namespace

bool mlp_general_supported(int L1, int L2) { return mlp_general_widths_ok(L1, L2) && !mlp_supported(L1, L2); }

int64_t mlp_general_param_count(int L1, int L2, int arena_align) { return goff(L1, L2, arena_align).NP; }

MLPGeneralLayout mlp_general_layout(int L1, int L2, int B) {
  MLPGeneralLayout lay{};
  const int L1p = pad32(L1), L2p = pad32(L2);  // the workspace keeps the padded extents
  lay.nslab = (B + kBC - 1) / kBC;
  lay.ncb = (L1 + kCB - 1) / kCB;
  lay.Bp = (int64_t)lay.nslab * kBC;
  lay.np_pad = (goff(L1, L2, 4).NP + 3) / 4 * 4;  // room for either arena packing
  // slices: tiles x slices about the chip's wave slots, whole 32-row K steps each (the wide rule)
  const int ntasks = gtasks(L1p, L2p), nk = (int)(lay.Bp / 32);
  int S = (kMLPWideWaveSlots + ntasks - 1) / ntasks;
  if (S > kMLPWideMaxSlices) S = kMLPWideMaxSlices;
  if (S > nk) S = nk;
  lay.slices = S < 1 ? 1 : S;
  const GPark pk = gpark(L1p, L2p, lay.Bp);
  lay.h1 = pk.h1;
  lay.park_elems = pk.total;
  lay.part_elems = (int64_t)lay.slices * lay.np_pad + (int64_t)lay.nslab * 4;
  lay.h1_elems = lay.Bp * L1p;
  return lay;
}

int launch_mlp_general_step(const MLPWideArgs& w_in, hipStream_t stream, int arena_align) {
  MLPWideArgs w = w_in;
  const MLPStepArgs& a = w.step;
  if (!mlp_general_widths_ok(a.L1, a.L2) || (arena_align != 1 && arena_align != 4)) return -1;
  if (a.B < 1 || a.B > kMLPWideMaxB) return -2;
  if (a.x_u8 && !mlp_input_affine_ok(a.x_scale, a.x_shift)) return -13;
  if (w.last_rows < 1 || w.last_rows > a.B || (!a.x_u8 && w.last_rows != a.B)) return -15;
  if (w.lr_mask < 0 || (w.lr_mask & (w.lr_mask + 1))) return -16;
  const MLPGeneralLayout lay = mlp_general_layout(a.L1, a.L2, a.B);
  if (!w.park || !w.part || !w.hdr || w.park_elems < lay.park_elems || w.part_elems < lay.part_elems) return -17;
  w.Bp = lay.Bp;
  w.np_pad = lay.np_pad;
  w.slab_stats = w.part + (int64_t)lay.slices * lay.np_pad;
  GenArgs g{};
  g.x_u8 = a.x_u8; g.x_f32 = a.x_f32; g.labels = a.labels; g.order = a.order; g.counters = a.counters;
  g.n_batches = a.n_batches;
  g.B = a.B; g.last_rows = w.last_rows; g.L1 = a.L1; g.L2 = a.L2;
  g.x_scale = a.x_scale; g.x_shift = a.x_shift;
  g.params = a.params;
  g.park = reinterpret_cast<__bf16*>(w.park);
  g.h1 = g.park + lay.h1;
  g.Bp = lay.Bp;
  g.hdr = w.hdr;
  g.slab_stats = w.slab_stats;
  g.align = arena_align;
  launch_forward<true>(g, lay.nslab, lay.ncb, stream);
  const int per = kPThreads / 64, ntasks = gtasks(pad32(a.L1), pad32(a.L2));
  const dim3 pgrid((ntasks + per - 1) / per, lay.slices);
  if (a.L1 % 32 || a.L2 % 32)
    hipLaunchKernelGGL(mlp_general_param_ragged_kernel, pgrid, dim3(kPThreads), 0, stream, w, arena_align);
  else hipLaunchKernelGGL(mlp_general_param_kernel, pgrid, dim3(kPThreads), 0, stream, w);
  // the apply is one thread per float of the arena: no alignment of a segment or of the total
  // enters it (the ragged parameter launch wrote zeros to the pads of an aligned arena in every
  // slice, so they see a zero gradient and stay zero)
  const int64_t np = goff(a.L1, a.L2, arena_align).NP;
  hipLaunchKernelGGL(mlp_wide_apply_kernel, dim3((unsigned)((np + kApplyThreads - 1) / kApplyThreads)),
                     dim3(kApplyThreads), 0, stream, w, np, lay.slices, lay.nslab);
  return 0;
}

int launch_mlp_general_eval(const MLPEvalArgs& a, uint16_t* h1, int64_t h1_elems, hipStream_t stream,
                            int arena_align) {
  if (!mlp_general_widths_ok(a.L1, a.L2) || (arena_align != 1 && arena_align != 4)) return -1;
  if (a.x_u8 && !mlp_input_affine_ok(a.x_scale, a.x_shift)) return -13;
  if (a.B <= 0) return 0;
  const MLPGeneralLayout lay = mlp_general_layout(a.L1, a.L2, a.B);
  if (!h1 || h1_elems < lay.h1_elems) return -17;
  GenArgs g{};
  g.x_u8 = a.x_u8; g.x_f32 = a.x_f32; g.labels = a.labels; g.order = a.index;
  g.B = a.B; g.last_rows = a.B; g.L1 = a.L1; g.L2 = a.L2;
  g.x_scale = a.x_scale; g.x_shift = a.x_shift;
  g.params = a.params;
  g.h1 = reinterpret_cast<__bf16*>(h1);
  g.Bp = lay.Bp;
  g.logits = a.logits; g.out = a.out; g.partials = a.partials;
  g.align = arena_align;
  launch_forward<false>(g, lay.nslab, lay.ncb, stream);
  return 0;
}

}  // namespace rla
