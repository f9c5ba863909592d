// gcs_mfma.h -- the matrix-core kernels of the submanifold convolution, for both operand types: float32 on
// v_mfma_f32_16x16x4_f32 (GCS_ENGINE_MFMA, include/gcs.h) and binary16 on v_mfma_f32_16x16x16_f16 (GCS_F16 of the `_t`
// entry points).  Top to bottom: the wave-tile geometry and the tile store that every kernel here shares, the float32
// gather-GEMM, the binary16 gather-GEMM, the tap-slice epilogue, the launch of the two GEMMs, then the weight gradient:
// one kernel for both operand types over a small operand type each.  Included by gcs_sparse.hip after k_subm_gemm (it
// uses KC, KR, half_t, tap_head and store_out); device code and launch helpers only, the plan, the workspace and the C
// ABI stay in gcs_sparse.hip.
//
// Contract of the forward and dX, the same as k_subm_gemm's: every output element is ONE fp32 chain from 0.0f over (tap
// in loop order, channel ascending), the bias added in fp32 after the chain, and the value converted to the element
// type ONCE, on the final store (store_out; no conversion for float32).  The same three workgroup tiles (gemm_tile),
// the same block-uniform tap skip (tap_head) and the same 16-channel LDS slices zero-padded beyond cin / nout / n.
//   float32   the f32-input MFMA is a k-ordered fmaf chain (one rounding per product, nothing wider inside), four MFMAs
//             of k = 4 channels per slice, so the kernel gives k_subm_gemm's values (tests/test_sparse_engine_gpu.py).
//   binary16  operands are read as binary16, every product is exact in fp32, a slice is ONE MFMA per accumulator.
//
// 256 threads = 4 waves.  A wave owns 16 x 16 (32 x 32 tile: waves 2 x 2) or 32 x 32 outputs (64 x 64: waves 2 x 2,
// 128 x 32: waves 4 x 1), that is 1 or 2 x 2 independent accumulators of 4 VGPRs; C/D of either MFMA is col = lane & 15,
// row = 4 * (lane >> 4) + reg.  The global loads of slice c + 1 are issued into registers before the MFMAs of slice c
// and stored to LDS after them.
//
// Tap slices: grid.z = S, slice s owns taps [s * per, min(K, (s + 1) * per)) of the loop order and, when S > 1, writes
// its fp32 partial tile to part[s][n][nout] -- always, zeros included, so what the workspace held before never matters;
// k_slice_epilogue then writes out = (sum of part[s], s ascending) + bias, 0 for the rows the mask excludes.  With
// S == 1 the kernel writes `out` itself, exactly as k_subm_gemm does.
#pragma once

namespace {

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

constexpr int kFragPitch = KC + 4;  // float32: words between rows of As (and of the forward's Bs)
constexpr int kHalfPitch = KC + 8;  // binary16: halves between rows of every LDS image
static_assert(KC == 16 && KR == 16, "binary16: a slice (a chunk) is four 4-half units per row and one MFMA deep");

// ---- what the kernels share ---------------------------------------------------------------------------------------
// The wave-tile geometry of a TM x TN workgroup tile: wave (wr, wc) is the tile-relative corner of the wave's WT x WT
// outputs, FR x FR fragments of 16 x 16; (fl, fk) = (lane & 15, lane >> 4) are the lane's coordinates in a fragment.
template <int TM, int TN>
struct WaveTile {
  static constexpr int WT = TM * TN == 32 * 32 ? 16 : 32;  // a wave's outputs: WT x WT
  static constexpr int FR = WT / 16;                       // 16 x 16 fragments per side
  static constexpr int WCOLS = TN / WT;
  static_assert((TM / WT) * WCOLS == 4, "four waves cover the tile");
  int wr, wc, fl, fk;
  __device__ __forceinline__ WaveTile() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wr = (wave / WCOLS) * WT;
    wc = (wave % WCOLS) * WT;
    fl = lane & 15;
    fk = lane >> 4;
  }
};

template <int FR>
__device__ __forceinline__ void clear_acc(mfma_f32x4 (&acc)[FR][FR]) {
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int j = 0; j < FR; j++) acc[i][j] = mfma_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

// The epilogue of a gather-GEMM workgroup: the wave's accumulators to the slice's partial tile or to y (store_out).
template <typename T, int TM, int TN, int FR>
__device__ __forceinline__ void store_tile(const WaveTile<TM, TN>& g, const mfma_f32x4 (&acc)[FR][FR], int64_t row0, int n0,
                                           int64_t n, int nout, const T* __restrict__ bias,
                                           const int32_t* __restrict__ rowmask, T* __restrict__ y, float* __restrict__ part) {
  float* pdst = part ? part + (int64_t)blockIdx.z * n * nout : nullptr;
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int64_t row = row0 + g.wr + 16 * i + 4 * g.fk + v;
      if (row >= n) continue;
      const bool zero = !part && rowmask && rowmask[row] != (int32_t)row;
#pragma unroll
      for (int j = 0; j < FR; j++) {
        const int o = n0 + g.wc + 16 * j + g.fl;
        if (o < nout) store_out(acc[i][j][v], row * nout + o, o, zero, bias, y, pdst);
      }
    }
}

// One binary16 MFMA per accumulator over two images that hold the reduction index contiguously, A[row][k] and B[col][k]
// at kHalfPitch: lane (fl, fk) holds A[row fl][k = 4 fk + j] and B[k = 4 fk + j][col fl], j = 0..3, one 8-byte fragment
// each.  At 24 halves (12 words) the 16 rows of a half-wave's fragment reads start at 16 different multiples of 4 words
// mod 64.  The step of the binary16 gather-GEMM (A = gathered rows, B = W) and of the binary16 dW (A = dY^T, B = X^T).
template <int TM, int TN, int FR>
__device__ __forceinline__ void mfma_step_h(const half_t* A, const half_t* B, const WaveTile<TM, TN>& g,
                                            mfma_f32x4 (&acc)[FR][FR]) {
  constexpr int P = kHalfPitch;
  h4 a[FR], b[FR];
#pragma unroll
  for (int i = 0; i < FR; i++) a[i] = *reinterpret_cast<const h4*>(&A[(g.wr + 16 * i + g.fl) * P + 4 * g.fk]);
#pragma unroll
  for (int j = 0; j < FR; j++) b[j] = *reinterpret_cast<const h4*>(&B[(g.wc + 16 * j + g.fl) * P + 4 * g.fk]);
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int j = 0; j < FR; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x16f16(a[i], b[j], acc[i][j], 0, 0, 0);
}

// ---- forward and dX, float32 ----------------------------------------------------------------------------------------
// Fragments come from LDS, one VGPR per operand:
//   A  lane holds A[row fl][k = fk]: the gathered rows, As[row][channel], pitch 20 words -- the 64 lanes of a fragment
//      read hit 64 different banks, and so do the 64 lanes of a staging write;
//   B  lane holds B[k = fk][col fl]: forward Bs[col][channel] at pitch 20 (W is read along channels), dX
//      Bs[channel][col] at pitch TN + 16 (W is read along columns): conflict-free both ways in both cases.
template <int TM, int TN, bool TRANS>
__global__ __launch_bounds__(256) void k_subm_gemm_mfma(const float* __restrict__ x, int cin, const float* __restrict__ w,
                                                        int64_t sk, int64_t sn, int64_t sc, const float* __restrict__ bias,
                                                        const int32_t* __restrict__ nbr, int K, int mirror,
                                                        const int32_t* __restrict__ rowmask, float* __restrict__ y, int nout,
                                                        int64_t n, int per, float* __restrict__ part) {
  constexpr int FR = WaveTile<TM, TN>::FR;
  constexpr int NA = TM * KC / 256, NB = TN * KC / 256;  // staged elements per thread
  constexpr int BPITCH = TRANS ? TN + 16 : kFragPitch;
  __shared__ float As[TM * kFragPitch];
  __shared__ float Bs[TRANS ? KC * BPITCH : TN * BPITCH];
  __shared__ int32_t sN[TM];
  const int tid = threadIdx.x;
  const WaveTile<TM, TN> g;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;
  const int kbeg = blockIdx.z * per, kend = kbeg + per < K ? kbeg + per : K;
  mfma_f32x4 acc[FR][FR];
  clear_acc(acc);

  for (int k = kbeg; k < kend; k++) {
    if (!tap_head<TM>(nbr, K, k, mirror, row0, n, sN)) continue;
    float ra[NA], rb[NB];
    auto fetch = [&](int c0) {
#pragma unroll
      for (int q = 0; q < NA; q++) {
        const int e = tid + q * 256, r = e / KC, c = c0 + e % KC;
        const int32_t j = sN[r];
        ra[q] = (j >= 0 && c < cin) ? x[(int64_t)j * cin + c] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < NB; q++) {
        const int e = tid + q * 256;
        const int cc = TRANS ? e / TN : e % KC, nn = TRANS ? e % TN : e / KC;
        const int c = c0 + cc, o = n0 + nn;
        rb[q] = (c < cin && o < nout) ? w[(int64_t)k * sk + (int64_t)o * sn + (int64_t)c * sc] : 0.0f;
      }
    };
    fetch(0);
    for (int c0 = 0; c0 < cin; c0 += KC) {
#pragma unroll
      for (int q = 0; q < NA; q++) {
        const int e = tid + q * 256;
        As[(e / KC) * kFragPitch + e % KC] = ra[q];
      }
#pragma unroll
      for (int q = 0; q < NB; q++) {
        const int e = tid + q * 256;
        const int cc = TRANS ? e / TN : e % KC, nn = TRANS ? e % TN : e / KC;
        Bs[TRANS ? cc * BPITCH + nn : nn * BPITCH + cc] = rb[q];
      }
      __syncthreads();
      if (c0 + KC < cin) fetch(c0 + KC);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float a[FR], b[FR];
#pragma unroll
        for (int i = 0; i < FR; i++) a[i] = As[(g.wr + 16 * i + g.fl) * kFragPitch + kk + g.fk];
#pragma unroll
        for (int j = 0; j < FR; j++)
          b[j] = TRANS ? Bs[(kk + g.fk) * BPITCH + g.wc + 16 * j + g.fl] : Bs[(g.wc + 16 * j + g.fl) * BPITCH + kk + g.fk];
#pragma unroll
        for (int i = 0; i < FR; i++)
#pragma unroll
          for (int j = 0; j < FR; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  store_tile(g, acc, row0, n0, n, nout, bias, rowmask, y, part);
}

// ---- forward and dX, binary16 ---------------------------------------------------------------------------------------
// Both LDS images are mfma_step_h's, As[row][channel] and Bs[column][channel].  The forward's W[o][k][:] is contiguous
// along the reduction and is staged in 8-byte units; dX reduces over cout, which W holds at stride K * cin, so dX reads
// W along its contiguous cin (coalesced) and stages it TRANSPOSED in LDS with 2-byte stores; nothing is transposed in
// the workspace.  Rows are cin (or cout) halves long with no multiple-of-anything requirement: the 8-byte global loads
// are taken only when the row stride is a multiple of 4 halves and the base is 8-byte aligned (`xvec`, `wvec`, decided
// on the host); otherwise every half is loaded on its own, guarded on its own.
__device__ __forceinline__ h4 h4_zero() { return h4{(half_t)0.0f, (half_t)0.0f, (half_t)0.0f, (half_t)0.0f}; }
// four halves at p, of which the first `valid` (1..4) exist; one 8-byte load when `vec` says stride and base allow it
__device__ __forceinline__ h4 load_h4(const half_t* __restrict__ p, int valid, int vec) {
  if (vec) return *reinterpret_cast<const h4*>(p);
  h4 v = h4_zero();
  v[0] = p[0];
  if (valid > 1) v[1] = p[1];
  if (valid > 2) v[2] = p[2];
  if (valid > 3) v[3] = p[3];
  return v;
}

template <int TM, int TN, bool TRANS>
__global__ __launch_bounds__(256) void k_subm_gemm_h(const half_t* __restrict__ x, int cin, int xvec,
                                                     const half_t* __restrict__ w, int64_t sk, int64_t sn, int64_t sc,
                                                     int wvec, const half_t* __restrict__ bias,
                                                     const int32_t* __restrict__ nbr, int K, int mirror,
                                                     const int32_t* __restrict__ rowmask, half_t* __restrict__ y, int nout,
                                                     int64_t n, int per, float* __restrict__ part) {
  constexpr int FR = WaveTile<TM, TN>::FR;
  constexpr int UA = TM * KC / 4, UB = TN * KC / 4;  // staged units of four halves
  constexpr int NA = (UA + 255) / 256, NB = (UB + 255) / 256;
  constexpr int P = kHalfPitch;
  __shared__ __attribute__((aligned(8))) half_t As[TM * P];
  __shared__ __attribute__((aligned(8))) half_t Bs[TN * P];
  __shared__ int32_t sN[TM];
  const int tid = threadIdx.x;
  const WaveTile<TM, TN> g;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;
  const int kbeg = blockIdx.z * per, kend = kbeg + per < K ? kbeg + per : K;
  mfma_f32x4 acc[FR][FR];
  clear_acc(acc);

  for (int k = kbeg; k < kend; k++) {
    if (!tap_head<TM>(nbr, K, k, mirror, row0, n, sN)) continue;
    h4 ra[NA], rb[NB];
    auto fetch = [&](int c0) {
#pragma unroll
      for (int q = 0; q < NA; q++) {
        const int e = tid + q * 256;
        h4 v = h4_zero();
        if (UA % 256 == 0 || e < UA) {
          const int r = e >> 2, c = c0 + 4 * (e & 3);
          const int32_t j = sN[r];
          if (j >= 0 && c < cin) v = load_h4(x + (int64_t)j * cin + c, cin - c, xvec);
        }
        ra[q] = v;
      }
#pragma unroll
      for (int q = 0; q < NB; q++) {
        const int e = tid + q * 256;
        h4 v = h4_zero();
        if (UB % 256 == 0 || e < UB) {
          if (!TRANS) {  // four reduction channels of one column: contiguous in W
            const int o = n0 + (e >> 2), c = c0 + 4 * (e & 3);
            if (o < nout && c < cin) v = load_h4(w + (int64_t)k * sk + (int64_t)o * sn + c, cin - c, wvec);
          } else {       // four columns of one reduction channel: contiguous in W
            const int c = c0 + e / (TN / 4), o = n0 + 4 * (e % (TN / 4));
            if (c < cin && o < nout) v = load_h4(w + (int64_t)k * sk + (int64_t)c * sc + o, nout - o, wvec);
          }
        }
        rb[q] = v;
      }
    };
    fetch(0);
    for (int c0 = 0; c0 < cin; c0 += KC) {
#pragma unroll
      for (int q = 0; q < NA; q++) {
        const int e = tid + q * 256;
        if (UA % 256 == 0 || e < UA) *reinterpret_cast<h4*>(&As[(e >> 2) * P + 4 * (e & 3)]) = ra[q];
      }
#pragma unroll
      for (int q = 0; q < NB; q++) {
        const int e = tid + q * 256;
        if (UB % 256 == 0 || e < UB) {
          if (!TRANS) {
            *reinterpret_cast<h4*>(&Bs[(e >> 2) * P + 4 * (e & 3)]) = rb[q];
          } else {
            const int cc = e / (TN / 4), nn = 4 * (e % (TN / 4));
#pragma unroll
            for (int t = 0; t < 4; t++) Bs[(nn + t) * P + cc] = rb[q][t];
          }
        }
      }
      __syncthreads();
      if (c0 + KC < cin) fetch(c0 + KC);
      mfma_step_h(As, Bs, g, acc);
      __syncthreads();
    }
  }
  store_tile(g, acc, row0, n0, n, nout, bias, rowmask, y, part);
}

// out[row][o] = T((sum of part[s][row][o], s ascending) + bias[o]); 0 where rowmask[row] != row
template <typename T>
__global__ void k_slice_epilogue(const float* __restrict__ part, int nslice, int64_t n, int nout, const T* __restrict__ bias,
                                 const int32_t* __restrict__ rowmask, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, len = n * nout;
  if (e >= len) return;
  const int64_t row = e / nout;
  const int o = (int)(e - row * nout);
  float v = part[e];
  for (int s = 1; s < nslice; s++) v += part[(int64_t)s * len + e];
  store_out(v, e, o, rowmask && rowmask[row] != (int32_t)row, bias, out, (float*)nullptr);
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// The launch of launch_gemm on the matrix cores, in S tap slices; `part` is fp32 [S][n][nout] when S > 1.  W's innermost
// extent is the real cin: the reduction of the forward, the columns of dX.
template <bool TRANS, typename T>
void launch_gemm_mfma(int tile, int S, const Gemm<T>& g, float* part, hipStream_t st) {
  const int per = (g.K + S - 1) / S;
  float* p = S > 1 ? part : nullptr;
  for_gemm_tile(tile, g.n, g.nout, S, [&](auto t, dim3 grid) {
    constexpr int TM = decltype(t)::TM, TN = decltype(t)::TN;
    if constexpr (sizeof(T) == 2) {
      const int xvec = g.cin % 4 == 0 && aligned8(g.x), wvec = (TRANS ? g.nout : g.cin) % 4 == 0 && aligned8(g.w);
      k_subm_gemm_h<TM, TN, TRANS><<<grid, 256, 0, st>>>(g.x, g.cin, xvec, g.w, g.sk, g.sn, g.sc, wvec, g.bias, g.nbr, g.K,
                                                         g.mirror, g.rowmask, g.y, g.nout, g.n, per, p);
    } else {
      k_subm_gemm_mfma<TM, TN, TRANS><<<grid, 256, 0, st>>>(g.x, g.cin, g.w, g.sk, g.sn, g.sc, g.bias, g.nbr, g.K, g.mirror,
                                                            g.rowmask, g.y, g.nout, g.n, per, p);
    }
  });
  if (S > 1) k_slice_epilogue<T><<<blocks_for(g.n * g.nout, 256), 256, 0, st>>>(part, S, g.n, g.nout, g.bias, g.rowmask, g.y);
}

// ---- dW -------------------------------------------------------------------------------------------------------------
// k_subm_dw on the matrix cores: part[s][o][k][c] = sum over the pairs p of slice s of tap k: dy[i_p][o] * x[nbr[i_p][k]][c].
// The grid, the slices [p0, p1) and the zero-filled last chunk are k_subm_dw's; every element is one fp32 chain from 0.0f
// over the slice's pairs in list order, KR pairs per chunk.  Square tiles, TILE = 64 or 32, waves 2 x 2.  With one slice
// (`part` null) the value is converted to T and stored to dw; otherwise the fp32 partial goes to part[s] and k_sum_slices
// converts after the sum over the slices.
// Three loads run ahead of the MFMAs of chunk c, none depending on another: the rows of x / dy of chunk c + 1, the nbr
// entries of chunk c + 2, the prow entries of chunk c + 3.  A thread stages NQ = TILE / 16 elements of each image, in
// the pairs r = tid / TILE + (256 / TILE) q at column tid % TILE (it loads along the channels, coalesced, single
// elements: every row stride and base is accepted), and keeps the indices of those pairs itself (a wave asks for one or
// two addresses).
// The LDS image of the two operands and the MFMAs of a chunk are the operand type's, DwOperand<T, TILE>:
//   SIZE             elements of one image
//   at(pair, col)    where the staged element of (pair, column) goes
//   step(D, X, g, acc)   the chunk's MFMAs: acc[row = o][col = c] += sum over the 16 pairs, in pair order
template <typename T, int TILE>
struct DwOperand;
// float32: pair-major images Ds[pair][o] and Xs[pair][c] at a pitch of TILE + 16 words: the 64 lanes of a fragment read
// (4 pairs x 16 columns) fall on 64 banks (pitch mod 64 = 16 or 48), a staging write is contiguous.  Four chained MFMAs
// per accumulator, k = 4 pairs each in pair order, continue k_subm_dw's fmaf chain: the two engines' dW is the same bits.
template <int TILE>
struct DwOperand<float, TILE> {
  static constexpr int PITCH = TILE + 16, SIZE = KR * PITCH;
  static __device__ __forceinline__ int at(int pair, int col) { return pair * PITCH + col; }
  template <int FR>
  static __device__ __forceinline__ void step(const float* Ds, const float* Xs, const WaveTile<TILE, TILE>& g,
                                              mfma_f32x4 (&acc)[FR][FR]) {
#pragma unroll
    for (int kk = 0; kk < KR; kk += 4) {
      float a[FR], b[FR];
#pragma unroll
      for (int i = 0; i < FR; i++) a[i] = Ds[(kk + g.fk) * PITCH + g.wr + 16 * i + g.fl];
#pragma unroll
      for (int j = 0; j < FR; j++) b[j] = Xs[(kk + g.fk) * PITCH + g.wc + 16 * j + g.fl];
#pragma unroll
      for (int i = 0; i < FR; i++)
#pragma unroll
        for (int j = 0; j < FR; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
};
// binary16: A[row = o][k = pair] and B[k = pair][col = c] both want four consecutive PAIRS of one channel on a lane, so
// the pair-major gathers are written to LDS transposed, Dt[o][pair] and Xt[c][pair]: mfma_step_h's images, one MFMA.
template <int TILE>
struct DwOperand<half_t, TILE> {
  static constexpr int PITCH = kHalfPitch, SIZE = TILE * PITCH;
  static __device__ __forceinline__ int at(int pair, int col) { return col * PITCH + pair; }
  template <int FR>
  static __device__ __forceinline__ void step(const half_t* Dt, const half_t* Xt, const WaveTile<TILE, TILE>& g,
                                              mfma_f32x4 (&acc)[FR][FR]) {
    mfma_step_h(Dt, Xt, g, acc);
  }
};

template <typename T, int TILE>
__global__ __launch_bounds__(256) void k_subm_dw_mfma(const T* __restrict__ dy, int cout, const T* __restrict__ x, int cin,
                                                      const int32_t* __restrict__ nbr, int K,
                                                      const int32_t* __restrict__ prow, const int32_t* __restrict__ hdr,
                                                      int64_t n, int nslice, float* __restrict__ part, T* __restrict__ dw) {
  static_assert(TILE == 32 || TILE == 64, "tile shape: one staging map serves both images");
  using Op = DwOperand<T, TILE>;
  constexpr int FR = WaveTile<TILE, TILE>::FR;
  constexpr int NQ = KR * TILE / 256, RSTEP = 256 / TILE;
  __shared__ __attribute__((aligned(8))) T Ds[Op::SIZE];
  __shared__ __attribute__((aligned(8))) T Xs[Op::SIZE];
  const int tid = threadIdx.x;
  const WaveTile<TILE, TILE> g;
  const int sr = tid / TILE, scol = tid % TILE;  // staging: pair sr + RSTEP * q, column scol
  const int tiles_c = (cin + TILE - 1) / TILE;
  const int o0 = (blockIdx.x / tiles_c) * TILE, c0 = (blockIdx.x % tiles_c) * TILE;
  const int k = blockIdx.y, s = blockIdx.z;
  const int64_t cnt = hdr[4 + k];
  const int64_t per = (cnt + nslice - 1) / nslice;
  const int64_t p0 = s * per, p1 = p0 + per < cnt ? p0 + per : cnt;
  mfma_f32x4 acc[FR][FR];
  clear_acc(acc);

  int32_t ia[NQ], ja[NQ], ib[NQ];  // (row, neighbour) of the chunk after this one; rows of the one after that
  T rd[NQ], rx[NQ];
  auto rows = [&](int64_t p, int32_t (&ii)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int64_t e = p + sr + RSTEP * q;
      ii[q] = e < p1 ? prow[(int64_t)k * n + e] : -1;
    }
  };
  auto nbrs = [&](const int32_t (&ii)[NQ], int32_t (&jj)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; q++) jj[q] = ii[q] >= 0 ? nbr[(int64_t)ii[q] * K + k] : -1;
  };
  auto fetch = [&]() {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      rd[q] = (ia[q] >= 0 && o0 + scol < cout) ? dy[(int64_t)ia[q] * cout + o0 + scol] : (T)0.0f;
      rx[q] = (ja[q] >= 0 && c0 + scol < cin) ? x[(int64_t)ja[q] * cin + c0 + scol] : (T)0.0f;
    }
  };
  rows(p0, ia);
  nbrs(ia, ja);
  fetch();
  rows(p0 + KR, ia);
  nbrs(ia, ja);
  rows(p0 + 2 * KR, ib);
  for (int64_t p = p0; p < p1; p += KR) {
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      Ds[Op::at(sr + RSTEP * q, scol)] = rd[q];
      Xs[Op::at(sr + RSTEP * q, scol)] = rx[q];
    }
    __syncthreads();
    fetch();
    nbrs(ib, ja);
#pragma unroll
    for (int q = 0; q < NQ; q++) ia[q] = ib[q];
    rows(p + 3 * KR, ib);
    Op::step(Ds, Xs, g, acc);
    __syncthreads();
  }
  float* out = part ? part + (int64_t)s * cout * K * cin : nullptr;
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int o = o0 + g.wr + 16 * i + 4 * g.fk + v;
      if (o >= cout) continue;
#pragma unroll
      for (int j = 0; j < FR; j++) {
        const int c = c0 + g.wc + 16 * j + g.fl;
        if (c < cin) store_out(acc[i][j][v], ((int64_t)o * K + k) * cin + c, 0, false, (const T*)nullptr, dw, out);
      }
    }
}

// the launch of k_subm_dw on the matrix cores: the same grid and slices; `part` is fp32 [S][cout][K][cin] when S > 1
template <typename T>
void launch_dw_mfma(int tile, int S, const T* dy, int cout, const T* x, int cin, const int32_t* nbr, int K,
                    const int32_t* prow, const int32_t* hdr, int64_t n, float* part, T* dw, hipStream_t st) {
  for_dw_tile(tile, cin, cout, K, S, [&](auto t, dim3 grid) {
    k_subm_dw_mfma<T, decltype(t)::TM><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S,
                                                             S > 1 ? part : nullptr, dw);
  });
}

}  // namespace
