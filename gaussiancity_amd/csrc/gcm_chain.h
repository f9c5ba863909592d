// gcm_chain.h -- the attribute head at inference in ONE launch per output key (gcm_head_chain, include/gcm.h): per row r of
// group g
//     f   = leaky(x[r] W1^T + onehots[r] Wma^T + b1)                 fc_1, fc_m_a, act
//     h   = leaky((f o alpha[g]) W2^T + beta[g] + bias2)             the key's hidden layer
//     out = transform(h Wout^T + bout)                               fc_out and k_head_out's transform
// with neither f nor h in memory.  Included by gcm_modlinear.hip after gcm_tile.h (the tile's constants, the accumulators,
// the epilogue nest) and after row_group; device code and the LDS carve only, the C ABI stays in gcm_modlinear.hip.
// DESIGN.md section 17b.
//
// A workgroup of 512 threads (8 waves as 2 x 4) owns T = 64 rows and walks the hidden width twice in chunks of CW = 256
// columns; a wave owns 32 rows x 64 columns, f4 acc[2][4].  (The other row-tile operators run 4 waves on 128 columns; here
// one workgroup fills a CU's LDS, so the second wave per SIMD is what covers the fragment reads and the barriers, and a
// chunk twice as wide halves the slices a row tile walks.  Chain of gcm_tile.h stages with 256 threads, so the product loop
// is written out below, in Chain's N-form and with its two barriers per slice.)
//   stage 1   per chunk one chain over the summed index [x | onehots]: I rounded up to 16, then K rounded up to 16, both
//             padded with zeros.  x and the weights come through LDS in 16-deep slices, the loads of slice s + 1 issued
//             before the MFMAs of slice s; x is read again per chunk (64 x I floats against 256 x I of weights).  The onehots
//             part is loaded element by element: K and its row stride need not be multiples of 4.  The epilogue adds b1,
//             applies LeakyReLU, multiplies by alpha[g] and writes the 64-row image of f o alpha into LDS (zeros for a row
//             beyond N or without a group, and for the columns H .. Hr).
//   stage 2   per chunk one chain over that image (H rounded up to 16), the epilogue adds beta[g], then bias2, applies
//             LeakyReLU and contracts the lane's 8 rows x 4 columns with Wout: po[row][c] = fmaf(h, wout[c][col], po) in
//             ascending column order of the lane, over the chunks in ascending order.  h is never stored.
//   the end   the 16 lanes of a row are added by a fixed exchange tree (xor 8, 4, 2, 1), the four column waves in
//             ascending order, then bout and the transform in double.  No float atomics; a row's bits depend on the row's
//             inputs alone, not on N, its place in the tile or the run.
// A wave whose 64 columns lie beyond the hidden width skips its MFMAs (narrow heads), never a barrier.
// LDS: the image of f at pitch Hr + 2 (b32 fragment reads of 16 rows x 2 k hit 32 different banks), a 256-column weight
// slice, a 64-row x slice: 157 184 bytes at H = 512, asked for through hipFuncSetAttribute.
#pragma once
#include <atomic>

namespace {

constexpr int kChainMaxHidden = 512;
constexpr int kChainMaxIn = 256;
constexpr int kChainMaxClasses = 32;
constexpr int kChainThreads = 512;
constexpr int CJ = 4;         // accumulators of a wave along the columns
constexpr int CW = 64 * CJ;   // hidden columns per chunk: four column waves of 16 CJ

__host__ __device__ constexpr int chain_round(int n) { return (n + KC - 1) / KC * KC; }
__host__ __device__ constexpr int chain_pitch(int H) { return chain_round(H) + 2; }
constexpr int kChainSliceWords = CW * kPitch;
size_t chain_lds_bytes(int H) { return (size_t)(kChainSliceWords + T * kPitch + T * chain_pitch(H)) * 4; }

struct ChainArgs {
  const float *x, *onehots, *w1, *b1, *wma, *w2, *alpha, *beta, *bias2, *wout, *bout;
  const int32_t* group;
  float* out;
  int64_t xs, os, w1s, w2s, N;
  int I, K, H, G, kind;
  float factor, slope;
};

// acc += A B^T over kext summed indices (a multiple of KC) for the workgroup's 64 rows and CW columns.  B comes through Ws
// in slices: w_at(column, k) returns four weights along k.  SLICED: A comes through Xs the same way, a_at(row, k); else A
// is the LDS image `image` (rows x summed index, pitch ap), read in place.  busy: the wave has columns to compute.  The
// first barrier orders the puts -- and what the caller wrote to the image -- before the fragment reads, the second keeps
// the next put, and what the caller writes afterwards, behind the last read (Chain::run's contract).
template <bool SLICED, typename AAt, typename WAt>
__device__ __forceinline__ void chain_product(f4 (&acc)[2][CJ], const WaveTile& g, bool busy, const float* image, int ap, int kext,
                                              float* Xs, float* Ws, AAt a_at, WAt w_at) {
  const int tid = threadIdx.x, sr = tid >> 2, sp = 4 * (tid & 3);  // piece sp of row sr (x: the first 256 threads), of the
  const bool stages_a = SLICED && tid < 4 * T;                     // weights' columns sr and sr + 128
  const int wcn = g.first_col<CJ>();
  const float* A = SLICED ? Xs : image;
  const int pitch = SLICED ? kPitch : ap;
  f4 va = zero4(), vb[2];
  auto fetch = [&](int k0) {
    if (stages_a) va = a_at(sr, k0 + sp);
    vb[0] = w_at(sr, k0 + sp);
    vb[1] = w_at(sr + 128, k0 + sp);
  };
  fetch(0);
  for (int k0 = 0; k0 < kext; k0 += KC) {
    if (stages_a) st4(&Xs[sr * kPitch + sp], va);
    st4(&Ws[sr * kPitch + sp], vb[0]);
    st4(&Ws[(sr + 128) * kPitch + sp], vb[1]);
    __syncthreads();
    if (k0 + KC < kext) fetch(k0 + KC);
    if (busy) {
      const int ka = SLICED ? 0 : k0;
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[CJ];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = A[(g.wr + 16 * i + g.fl) * pitch + ka + kk + g.fk];
#pragma unroll
        for (int j = 0; j < CJ; j++) fb[j] = Ws[(wcn + 16 * j + g.fl) * kPitch + kk + g.fk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < CJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
}

template <int NC>
__global__ __launch_bounds__(kChainThreads) void k_head_chain(const ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float chain_lds[];
  float* Ws = chain_lds;                 // a slice of the weights: 256 columns x 16
  float* Xs = Ws + kChainSliceWords;     // a slice of x: 64 rows x 16; at the end the column waves' sums
  float* Fs = Xs + T * kPitch;           // f o alpha: 64 rows x Hr
  __shared__ int32_t sG[T];
  const int tid = threadIdx.x, wave = tid >> 6;
  WaveTile g;  // 8 waves as 2 x 4: the wave's 32 rows and, through first_col<CJ>, its 64 columns
  g.wr = (wave >> 2) * 32;
  g.wc = (wave & 3) * 32;
  const int wcn = g.first_col<CJ>();
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int I = a.I, K = a.K, H = a.H;
  const int Ir = chain_round(I), KT = Ir + chain_round(K), Hr = chain_round(H), FP = chain_pitch(H);
  const float slope = a.slope;
  if (tid < T) sG[tid] = row0 + tid < a.N ? row_group(a.group, row0 + tid, a.G) : -1;
  __syncthreads();

  // ---- stage 1: f o alpha -> Fs ---------------------------------------------------------------------------------------
  auto x_at = [&](int r, int k) {  // four of [x | onehots] of row r along the summed index
    f4 v = zero4();
    const int64_t row = row0 + r;
    if (row >= a.N) return v;
    if (k < Ir) {
      if (k < I) v = ld4(a.x + row * a.xs + k);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++)
        if (k - Ir + e < K) v[e] = a.onehots[row * a.os + k - Ir + e];
    }
    return v;
  };
  for (int n0 = 0; n0 < Hr; n0 += CW) {
    auto w1_at = [&](int col, int k) {  // four of [W1 | Wma] of hidden column n0 + col
      f4 v = zero4();
      const int c = n0 + col;
      if (c >= H) return v;
      if (k < Ir) {
        if (k < I) v = ld4(a.w1 + (int64_t)c * a.w1s + k);
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (k - Ir + e < K) v[e] = a.wma[(int64_t)c * K + k - Ir + e];
      }
      return v;
    };
    f4 acc[2][CJ];
    clear_acc(acc);
    chain_product<true>(acc, g, n0 + wcn < Hr, nullptr, 0, KT, Xs, Ws, x_at, w1_at);
    for_each_output(acc, g, [&](int rl, int cl, float v) {
      const int c = n0 + cl;
      if (c >= Hr) return;
      const int gr = sG[rl];
      float f = 0.0f;
      if (c < H && gr >= 0) {
        f = v + a.b1[c];
        f = f > 0.0f ? f : f * slope;
        if (a.alpha) f *= a.alpha[(int64_t)gr * H + c];
      }
      Fs[rl * FP + c] = f;
    });
  }

  // ---- stage 2: h = leaky(Fs W2^T + beta[g] + bias2), contracted with Wout as it appears -------------------------------
  float po[2][4][NC];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++)
#pragma unroll
      for (int c = 0; c < NC; c++) po[i][v][c] = 0.0f;
  for (int n0 = 0; n0 < H; n0 += CW) {
    auto w2_at = [&](int col, int k) { return (n0 + col < H && k < H) ? ld4(a.w2 + (int64_t)(n0 + col) * a.w2s + k) : zero4(); };
    f4 acc[2][CJ];
    clear_acc(acc);
    chain_product<false>(acc, g, n0 + wcn < H, Fs, FP, Hr, Xs, Ws, [](int, int) { return zero4(); }, w2_at);
    float wo[CJ][NC], bj[CJ];
#pragma unroll
    for (int j = 0; j < CJ; j++) {
      const int c = n0 + wcn + 16 * j + g.fl;
      bj[j] = (a.bias2 && c < H) ? a.bias2[c] : 0.0f;
#pragma unroll
      for (int q = 0; q < NC; q++) wo[j][q] = c < H ? a.wout[(int64_t)q * H + c] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int gr = sG[g.wr + 16 * i + 4 * g.fk + v];
        if (gr < 0) continue;
#pragma unroll
        for (int j = 0; j < CJ; j++) {
          const int c = n0 + wcn + 16 * j + g.fl;
          if (c >= H) continue;
          float h = acc[i][j][v];
          if (a.beta) h += a.beta[(int64_t)gr * H + c];
          if (a.bias2) h += bj[j];
          h = h > 0.0f ? h : h * slope;
#pragma unroll
          for (int q = 0; q < NC; q++) po[i][v][q] = fmaf(h, wo[j][q], po[i][v][q]);
        }
      }
  }

  // ---- the end: the row's 16 lanes, the four column waves, the transform -----------------------------------------------
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++)
#pragma unroll
      for (int q = 0; q < NC; q++)
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) po[i][v][q] += __shfl_xor(po[i][v][q], m, 64);
  float* Ex = Xs;  // [3 column waves][64 rows][4] (the x slice is not read after stage 1)
  const int cw = wave & 3;
  if (cw != 0 && g.fl == 0) {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int v = 0; v < 4; v++)
#pragma unroll
        for (int q = 0; q < NC; q++) Ex[((cw - 1) * T + g.wr + 16 * i + 4 * g.fk + v) * 4 + q] = po[i][v][q];
  }
  __syncthreads();
  if (cw != 0 || g.fl != 0) return;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int rl = g.wr + 16 * i + 4 * g.fk + v;
      const int64_t row = row0 + rl;
      if (row >= a.N) continue;
      const int gr = sG[rl];
#pragma unroll
      for (int q = 0; q < NC; q++) {
        float res = 0.0f;
        if (gr >= 0) {
          float s = po[i][v][q];
#pragma unroll
          for (int w = 0; w < 3; w++) s += Ex[(w * T + rl) * 4 + q];
          const float t = a.bout ? s + a.bout[q] : s;
          const double sg = 1.0 / (1.0 + exp(-(double)t));
          double d;
          if (a.kind == GCM_SCALE) d = 1.0 + (double)fminf(fmaxf(t, -1.0f), 1.0f) * (double)a.factor;
          else if (a.kind == GCM_OPACITY) d = sg * (double)a.factor + (1.0 - (double)a.factor);
          else d = (sg - 0.5) * (double)a.factor;
          res = (float)d;
        }
        a.out[row * NC + q] = res;
      }
    }
}

// more than 64 KB of dynamic LDS has to be asked for, per kernel and per device (asking twice is harmless)
hipError_t chain_lds_attr() {
  constexpr int kDevices = 64;
  static std::atomic<bool> done[kDevices];
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < kDevices;
  if (known && done[dev].load(std::memory_order_acquire)) return hipSuccess;
  const void* fns[2] = {(const void*)k_head_chain<1>, (const void*)k_head_chain<3>};
  for (const void* f : fns) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)chain_lds_bytes(kChainMaxHidden));
    if (e != hipSuccess) return e;
  }
  if (known) done[dev].store(true, std::memory_order_release);
  return hipSuccess;
}

}  // namespace
