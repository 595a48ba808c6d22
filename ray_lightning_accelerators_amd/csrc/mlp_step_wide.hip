// Wide-batch training step of the MNIST classifier MLP (784 -> L1 -> L2 -> 10) for gfx950:
// 256 < B <= 4096 rows, where the step is a set of real GEMMs (layer 1: B x 784 x L1, dW1:
// 784 x L1 over K = B) and the one-CU-per-32-rows chain of mlp_step3.hip no longer fits.
// Same contract as mlp_kernels.hip's mlp_train_step; three launches, every reduction in a
// fixed order (no float atomics), so two runs from one state -- eager or replayed from a
// captured graph -- agree bit for bit.
//
//   1. slab   one 512-thread workgroup per 64 batch rows.  The slab's pixels are staged into a
//             padded LDS image (64 x 808 bf16, 101 KB) as bf16(fmaf(u8, x_scale, x_shift)) or
//             from fp32 rows; layer 1 runs on v_mfma_f32_16x16x32_bf16 with each wave holding
//             whole-K fp32 accumulators of its (row tile, column tile) pairs and W1 streamed
//             from the fp32 master in 32-wide K chunks (converted where it is staged -- no
//             bf16 shadow, no fixed point, no clamp).  The X image is dead after layer 1, so
//             H1, H2, the logits and dZ alias it.  Softmax / NLL / accuracy, dZ (scaled by
//             1 / rows of the batch, read against the device cursor), dH2 and dH1 follow in
//             LDS and registers.  Everything the parameter launch contracts over the batch is
//             parked in HBM TRANSPOSED, [feature][Bp] bf16 (XT, H1T, H2T, dH2T, dZT, dH1T):
//             the accumulator fragment of a 16x16 MFMA tile is four consecutive batch rows of
//             one feature, i.e. one 8-byte store, and the next launch's operand fragments
//             become plain 16-byte loads of 8 consecutive batch rows -- no LDS and no
//             transposed read there at all.  The slab files (sum NLL, #correct, #rows).
//   2. param  one wave per 16x16 gradient tile and batch slice: dW1 (49 x L1/16 tiles), dW2,
//             dW3 and the three biases (the same MFMA against a fragment of ones).  The batch
//             is cut into S slices of whole 32-row K steps, S chosen so that tiles x S covers
//             the chip's wave slots; slice s writes its fp32 partial to part[s].
//   3. apply  one thread per parameter sums the S partials in slice order and runs the
//             epilogue -- Adam / AdamW (mlp_common.h adam1, the rate from lr_tensor[(t - 1) &
//             lr_mask] when given), += grads, or a plain store.  One lane adds the slab rows
//             in slab order into the stats ring and advances counters[0] / counters[1].
//             (A short third launch instead of a ticket + finisher in launch 2: it needs no
//             device-scope fence or self-resetting counter, and under a captured graph its cost
//             is one more node.)
//
// Launch 1 only READS counters and launch 3 is the only writer: slab 0 leaves (t, cursor, rows)
// in the workspace header, which launch 3's blocks read, so no block can see an advanced
// counter of its own step.
#include "common.h"
#include "kernels.h"
#include "mlp_apply.h"
#include "mlp_common.h"

namespace rla {
namespace {

using namespace mlp;

constexpr int kBC = 64;          // rows per slab
constexpr int kXS = 808;         // LDS row stride of X (bf16): rows 20 dwords apart, conflict-free b128
constexpr int kKS1 = 25;         // ceil(784 / 32) K steps of layer 1
constexpr int kThreads = 512;    // slab launch: 8 waves
constexpr int kWaves = kThreads / 64;
constexpr int kMT = kBC / 16;    // 16-row tiles per slab
constexpr int kDZS = 40;         // LDS row stride of dZ (K padded to 32 + 8)
constexpr int kPThreads = 256;   // param / apply launches

template <int L1, int L2>
struct WCfg {
  static constexpr int H1S = L1 + 8, H2S = L2 + 8, TN1 = L1 / 16, TN2 = L2 / 16;
  static constexpr size_t szX = (size_t)kBC * kXS * 2;
  // aliases of the X image, live after layer 1
  static constexpr size_t oH1 = 0;
  static constexpr size_t oH2 = oH1 + (size_t)kBC * H1S * 2;
  static constexpr size_t oZ = oH2 + (size_t)kBC * H2S * 2;
  static constexpr size_t odZ = oZ + (size_t)kBC * 16 * 4;
  static constexpr size_t endAlias = odZ + (size_t)kBC * kDZS * 2;
  static constexpr size_t oY = szX;
  static constexpr size_t total = oY + kBC * 4;
  static_assert(endAlias <= szX, "H1 / H2 / Z / dZ must fit the dead X image");
  static_assert(L1 % 32 == 0 && L2 % 32 == 0 && L1 <= 128 && L2 <= 256, "layer widths");
  static_assert(TN1 % 2 == 0, "two wave groups share the column tiles of layer 1");
};

// Parked operands, [feature][Bp] bf16 each, in this order (element offsets).
struct Park {
  int64_t xt, h1t, h2t, dh2t, dzt, dh1t, total;
};
inline __host__ __device__ Park park_layout(int L1, int L2, int64_t Bp) {
  Park p;
  p.xt = 0;
  p.h1t = p.xt + kD * Bp;
  p.h2t = p.h1t + L1 * Bp;
  p.dh2t = p.h2t + L2 * Bp;
  p.dzt = p.dh2t + L2 * Bp;
  p.dh1t = p.dzt + 16 * Bp;
  p.total = p.dh1t + L1 * Bp;
  return p;
}

__device__ __forceinline__ void st4(__bf16* p, bf16x4 v) { *reinterpret_cast<bf16x4*>(p) = v; }

// ---------------------------------------------------------------------------------------
// Launch 1: the slab.
// ---------------------------------------------------------------------------------------
template <int L1, int L2, bool U8>
__global__ __launch_bounds__(kThreads) void mlp_wide_slab_kernel(MLPWideArgs w) {
  using C = WCfg<L1, L2>;
  const MLPStepArgs& a = w.step;
  __shared__ __attribute__((aligned(16))) char smem[C::total];
  __bf16* sX = (__bf16*)smem;
  __bf16* sH1 = (__bf16*)(smem + C::oH1);
  __bf16* sH2 = (__bf16*)(smem + C::oH2);
  float* sZ = (float*)(smem + C::oZ);
  __bf16* sdZ = (__bf16*)(smem + C::odZ);
  int* sY = (int*)(smem + C::oY);

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const int slab = blockIdx.x, row0 = slab * kBC;
  const int64_t Bp = (int64_t)gridDim.x * kBC;
  const Park pk = park_layout(L1, L2, Bp);
  __bf16* park = reinterpret_cast<__bf16*>(w.park);

  // batch position and size from the device state (a captured graph replays at any cursor)
  const int64_t cursor = (U8 && a.counters) ? a.counters[1] : 0;
  const int rows = (U8 && cursor == a.n_batches - 1) ? w.last_rows : a.B;
  const int nvalid = min(kBC, max(0, rows - row0));
  const int64_t* idx = U8 ? a.order + cursor * a.B : nullptr;
  if (slab == 0 && tid == 0) {
    w.hdr[0] = (a.counters ? a.counters[0] : 0) + 1;
    w.hdr[1] = cursor;
    w.hdr[2] = rows;
  }

  // ---- stage the slab's rows as bf16 (rows past the batch: zero pixels, label -1) ----
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
  if (tid < kBC) {
    int y = -1;
    if (tid < nvalid) y = (int)(U8 ? a.labels[idx[row0 + tid]] : a.labels[row0 + tid]);
    sY[tid] = y;
  }
  __syncthreads();

  // ---- park X^T: 8 consecutive rows of one pixel per 16-byte store ----
  for (int t = tid; t < kD * (kBC / 8); t += kThreads) {
    const int c = t & 7, pix = t >> 3;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = sX[(c * 8 + j) * kXS + pix];
    *reinterpret_cast<bf16x8*>(park + pk.xt + (int64_t)pix * Bp + row0 + c * 8) = v;
  }

  const float* W1 = a.params + Off<L1, L2>::W1;
  const float* b1 = a.params + Off<L1, L2>::B1;
  const float* W2 = a.params + Off<L1, L2>::W2;
  const float* b2 = a.params + Off<L1, L2>::B2;
  const float* W3 = a.params + Off<L1, L2>::W3;
  const float* b3 = a.params + Off<L1, L2>::B3;

  // ---- layer 1: wave wv owns row tile wv & 3 and column tiles (wv >> 2) + 2 j, whole K ----
  constexpr int NTW = C::TN1 / 2;
  const int mt1 = wv & 3, ct0 = wv >> 2;
  f32x4 acc1[NTW];
#pragma unroll
  for (int j = 0; j < NTW; ++j) acc1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
  for (int ks = 0; ks < kKS1; ++ks) {
    const int k = ks * 32 + 8 * g;
    const bf16x8 afrag = ld8(sX + (mt1 * 16 + r16) * kXS + k);
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      bf16x8 bfrag = zero8();
      if (k < kD) {
        const float* wrow = W1 + (int64_t)((ct0 + 2 * j) * 16 + r16) * kD + k;
        bfrag = cvt8(ld4(wrow), ld4(wrow + 4));
      }
      acc1[j] = mfma16(afrag, bfrag, acc1[j]);
    }
  }
  __syncthreads();  // the X image is dead: H1 / H2 / Z / dZ take its place
#pragma unroll
  for (int j = 0; j < NTW; ++j) {
    const int n = (ct0 + 2 * j) * 16 + r16;
    const float bias = b1[n];
    bf16x4 t4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __bf16 h = (__bf16)fmaxf(acc1[j][i] + bias, 0.f);
      sH1[(mt1 * 16 + 4 * g + i) * C::H1S + n] = h;
      t4[i] = h;
    }
    st4(park + pk.h1t + (int64_t)n * Bp + row0 + mt1 * 16 + 4 * g, t4);
  }
  __syncthreads();

  // ---- layer 2 ----
  for (int tile = wv; tile < kMT * C::TN2; tile += kWaves) {
    const int mt = tile % kMT, nt = tile / kMT;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float* wrow = W2 + (nt * 16 + r16) * L1;
#pragma unroll
    for (int ks = 0; ks < L1 / 32; ++ks) {
      const int k = ks * 32 + 8 * g;
      const bf16x8 bfrag = cvt8(ld4(wrow + k), ld4(wrow + k + 4));
      acc = mfma16(ld8(sH1 + (mt * 16 + r16) * C::H1S + k), bfrag, acc);
    }
    const int n = nt * 16 + r16;
    const float bias = b2[n];
    bf16x4 t4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __bf16 h = (__bf16)fmaxf(acc[i] + bias, 0.f);
      sH2[(mt * 16 + 4 * g + i) * C::H2S + n] = h;
      t4[i] = h;
    }
    st4(park + pk.h2t + (int64_t)n * Bp + row0 + mt * 16 + 4 * g, t4);
  }
  __syncthreads();

  // ---- layer 3 (classes padded to 16) ----
  if (wv < kMT) {
    const int mt = wv;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < L2 / 32; ++ks) {
      const int k = ks * 32 + 8 * g;
      bf16x8 bfrag = zero8();
      if (r16 < kNC) bfrag = cvt8(ld4(W3 + r16 * L2 + k), ld4(W3 + r16 * L2 + k + 4));
      acc = mfma16(ld8(sH2 + (mt * 16 + r16) * C::H2S + k), bfrag, acc);
    }
    if (r16 < kNC) {
      const float bias = b3[r16];
#pragma unroll
      for (int i = 0; i < 4; ++i) sZ[(mt * 16 + 4 * g + i) * 16 + r16] = acc[i] + bias;
    }
  }
  __syncthreads();

  // ---- log-softmax / NLL / accuracy / dZ: wave 0, one lane per row ----
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
      loss = m + logf(sum) - z[y];
      hit = (arg == y) ? 1.f : 0.f;
      cnt = 1.f;
#pragma unroll
      for (int j = 0; j < kNC; ++j) d8[j >> 3][j & 7] = (__bf16)((p[j] * inv - (j == y ? 1.f : 0.f)) * inv_rows);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x8*>(sdZ + r * kDZS + 8 * q) = d8[q];
#pragma unroll
    for (int j = 0; j < 16; ++j) park[pk.dzt + (int64_t)j * Bp + row0 + r] = d8[j >> 3][j & 7];
    // fixed butterfly: the same tree in every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      loss += __shfl_down(loss, off, 64);
      hit += __shfl_down(hit, off, 64);
      cnt += __shfl_down(cnt, off, 64);
    }
    if (lane == 0) {
      float* st = w.slab_stats + slab * 4;
      st[0] = loss; st[1] = hit; st[2] = cnt; st[3] = 0.f;
    }
  }
  __syncthreads();

  // ---- dH2 = (dZ W3) * (H2 > 0): in place of H2, and parked transposed ----
  for (int tile = wv; tile < kMT * C::TN2; tile += kWaves) {
    const int mt = tile % kMT, nt = tile / kMT, n = nt * 16 + r16;
    const bf16x8 afrag = ld8(sdZ + (mt * 16 + r16) * kDZS + 8 * g);
    bf16x8 bfrag = zero8();
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int j = 8 * g + jj;
      if (j < kNC) bfrag[jj] = (__bf16)W3[j * L2 + n];
    }
    const f32x4 acc = mfma16(afrag, bfrag, f32x4{0.f, 0.f, 0.f, 0.f});
    bf16x4 t4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __bf16* hp = sH2 + (mt * 16 + 4 * g + i) * C::H2S + n;
      const __bf16 d = ((float)(*hp) > 0.f) ? (__bf16)acc[i] : (__bf16)0.f;
      *hp = d;
      t4[i] = d;
    }
    st4(park + pk.dh2t + (int64_t)n * Bp + row0 + mt * 16 + 4 * g, t4);
  }
  __syncthreads();

  // ---- dH1 = (dH2 W2) * (H1 > 0), parked transposed ----
  for (int tile = wv; tile < kMT * C::TN1; tile += kWaves) {
    const int mt = tile % kMT, ct = tile / kMT, m = ct * 16 + r16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < L2 / 32; ++ks) {
      const int k = ks * 32 + 8 * g;
      bf16x8 bfrag;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) bfrag[jj] = (__bf16)W2[(k + jj) * L1 + m];
      acc = mfma16(ld8(sH2 + (mt * 16 + r16) * C::H2S + k), bfrag, acc);
    }
    bf16x4 t4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const __bf16 hv = sH1[(mt * 16 + 4 * g + i) * C::H1S + m];
      t4[i] = ((float)hv > 0.f) ? (__bf16)acc[i] : (__bf16)0.f;
    }
    st4(park + pk.dh1t + (int64_t)m * Bp + row0 + mt * 16 + 4 * g, t4);
  }
}

// ---------------------------------------------------------------------------------------
// Launch 2: one wave per (gradient tile, batch slice).  D[i][j] = sum_b A^T[i][b] B^T[j][b]
// over the slice's K steps; lane (r16, g) holds D[4 g + i][r16].
// ---------------------------------------------------------------------------------------
template <int L1, int L2>
__global__ __launch_bounds__(kPThreads) void mlp_wide_param_kernel(MLPWideArgs w) {
  using O = Off<L1, L2>;
  constexpr int TN1 = L1 / 16, TN2 = L2 / 16;
  constexpr int NT_W1 = kTiles * TN1, NT_W2 = TN2 * TN1, NT_W3 = TN2, NT_B = TN1 + TN2 + 1;
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
  const int task = blockIdx.x * (kPThreads / 64) + (threadIdx.x >> 6);
  if (task >= NT_W1 + NT_W2 + NT_W3 + NT_B) return;  // whole waves; the kernel has no barrier
  const int s = blockIdx.y, S = gridDim.y;
  const int64_t Bp = w.Bp;
  const int nk = (int)(Bp / 32);
  const int ks0 = (int)((int64_t)s * nk / S), ks1 = (int)((int64_t)(s + 1) * nk / S);
  const Park pk = park_layout(L1, L2, Bp);
  const __bf16* park = reinterpret_cast<const __bf16*>(w.park);
  float* out = w.part + (int64_t)s * w.np_pad;

  const __bf16* arow;         // A^T row of this lane
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
  if (kind == 0) {
    *reinterpret_cast<F4*>(out + O::W1 + (int64_t)(t1 * 16 + r16) * kD + t0 * 16 + 4 * g) =
        F4{{acc[0], acc[1], acc[2], acc[3]}};
  } else if (kind == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[O::W2 + (int64_t)(t0 * 16 + 4 * g + i) * L1 + t1 * 16 + r16] = acc[i];
  } else if (kind == 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (4 * g + i < kNC) out[O::W3 + (int64_t)(4 * g + i) * L2 + t0 * 16 + r16] = acc[i];
  } else if (r16 == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * g + i;
      if (t0 < TN1) out[O::B1 + t0 * 16 + e] = acc[i];
      else if (t0 < TN1 + TN2) out[O::B2 + (t0 - TN1) * 16 + e] = acc[i];
      else if (e < kNC) out[O::B3 + e] = acc[i];
    }
  }
}

// Launch 3 (slices summed in slice order, the epilogue, the stats row and the counters) is
// mlp_wide_apply_kernel of mlp_apply.h, shared with mlp_step_general.hip.

template <int L1, int L2>
int dispatch_wide(const MLPWideArgs& w, const MLPWideLayout& lay, hipStream_t stream) {
  constexpr int ntasks = kTiles * (L1 / 16) + (L2 / 16) * (L1 / 16) + L2 / 16 + L1 / 16 + L2 / 16 + 1;
  const int per = kPThreads / 64;
  if (w.step.x_u8)
    hipLaunchKernelGGL((mlp_wide_slab_kernel<L1, L2, true>), dim3(lay.nslab), dim3(kThreads), 0, stream, w);
  else
    hipLaunchKernelGGL((mlp_wide_slab_kernel<L1, L2, false>), dim3(lay.nslab), dim3(kThreads), 0, stream, w);
  hipLaunchKernelGGL((mlp_wide_param_kernel<L1, L2>), dim3((ntasks + per - 1) / per, lay.slices), dim3(kPThreads), 0,
                     stream, w);
  const int64_t np = Off<L1, L2>::NP;
  hipLaunchKernelGGL(mlp_wide_apply_kernel, dim3((unsigned)((np + kPThreads - 1) / kPThreads)), dim3(kPThreads), 0,
                     stream, w, np, lay.slices, lay.nslab);
  return 0;
}

#define RLA_MLP_SHAPES(X) \
  X(32, 32) X(32, 64) X(32, 128) X(32, 256) \
  X(64, 64) X(64, 128) X(64, 256) \
  X(128, 128) X(128, 256) X(128, 64)

}  // namespace

MLPWideLayout mlp_wide_layout(int L1, int L2, int B) {
  MLPWideLayout lay{};
  lay.nslab = (B + kBC - 1) / kBC;
  lay.Bp = (int64_t)lay.nslab * kBC;
  const int64_t np = (int64_t)L1 * kD + L1 + (int64_t)L2 * L1 + L2 + kNC * L2 + kNC;
  lay.np_pad = (np + 3) / 4 * 4;
  // slices: tiles x slices about the chip's wave slots (256 CUs x 4), whole 32-row K steps each
  const int ntasks = kTiles * (L1 / 16) + (L2 / 16) * (L1 / 16) + L2 / 16 + L1 / 16 + L2 / 16 + 1;
  const int nk = (int)(lay.Bp / 32);
  int S = (kMLPWideWaveSlots + ntasks - 1) / ntasks;
  if (S > kMLPWideMaxSlices) S = kMLPWideMaxSlices;
  if (S > nk) S = nk;
  lay.slices = S < 1 ? 1 : S;
  lay.park_elems = park_layout(L1, L2, lay.Bp).total;
  lay.part_elems = (int64_t)lay.slices * lay.np_pad + (int64_t)lay.nslab * 4;
  return lay;
}

int launch_mlp_wide_step(const MLPWideArgs& w_in, hipStream_t stream) {
  MLPWideArgs w = w_in;
  const MLPStepArgs& a = w.step;
  if (!mlp_supported(a.L1, a.L2)) return -1;
  if (a.B <= kMLPWideMinB - 1 || a.B > kMLPWideMaxB) return -2;
  if (a.x_u8 && !mlp_input_affine_ok(a.x_scale, a.x_shift)) return -13;
  if (w.last_rows < 1 || w.last_rows > a.B || (!a.x_u8 && w.last_rows != a.B)) return -15;
  if (w.lr_mask < 0 || (w.lr_mask & (w.lr_mask + 1))) return -16;
  const MLPWideLayout lay = mlp_wide_layout(a.L1, a.L2, a.B);
  if (!w.park || !w.part || !w.hdr || w.park_elems < lay.park_elems || w.part_elems < lay.part_elems) return -17;
  w.Bp = lay.Bp;
  w.np_pad = lay.np_pad;
  w.slab_stats = w.part + (int64_t)lay.slices * lay.np_pad;
#define RLA_CASE(a1, a2) if (a.L1 == a1 && a.L2 == a2) return dispatch_wide<a1, a2>(w, lay, stream);
  RLA_MLP_SHAPES(RLA_CASE)
#undef RLA_CASE
  return -1;
}

}  // namespace rla
