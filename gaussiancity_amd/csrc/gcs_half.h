// gcs_half.h -- the binary16 path of libgcs_hip.so (GCS_F16 of the `_t` entry points, include/gcs.h): the submanifold
// convolution's three products on v_mfma_f32_16x16x16_f16, the binary16 variants of the fold of dY, of dB and of the slice
// sums, and segment_csr.  Included by gcs_sparse.hip after its kernels (it uses KC, KR, mfma_f32x4 and seg_bounds);
// device code and launch helpers only, the plan, the workspace and the C ABI stay in gcs_sparse.hip.
//
// Contract (gcs.h): operands are read as binary16, every product is exact in fp32, every sum is
// fp32 in a fixed order (inside the matrix cores, across taps, chunks and slices), the bias is added in fp32 after the
// sum, and the value is rounded to binary16 ONCE, on the final store.  Partial tiles and partial dW / dB are fp32.
//
// Forward and dX: k_subm_gemm_h is k_subm_gemm_mfma with binary16 operands -- the same three workgroup tiles, the same
// block-uniform tap skip, the same tap slices and 16-channel LDS slices zero-padded beyond cin / nout / n, `mirror` and
// `rowmask` for dX.  One 16-channel slice is ONE MFMA per accumulator.  Operand maps, lane l, fl = l & 15, fk = l >> 4:
//   A[row fl][k = 4 fk + j], B[k = 4 fk + j][col fl] (j = 0..3: one 8-byte fragment), C/D[row 4 fk + r][col fl].
// Both LDS images hold the reduction index contiguously, As[row][channel] and Bs[column][channel], at a pitch of 24
// halves (12 words): the 16 rows of a half-wave's 8-byte fragment reads start at 16 different multiples of 4 words
// mod 64.  The forward's W[o][k][:] is contiguous along the reduction and is staged in 8-byte units; dX reduces over
// cout, which W holds at stride K * cin, so dX reads W along its contiguous cin (coalesced) and stages it TRANSPOSED in
// LDS with 2-byte stores; nothing is transposed in the workspace.
// Rows are cin (or cout) halves long with no multiple-of-anything requirement: the 8-byte global loads are taken only
// when the row stride is a multiple of 4 halves and the base is 8-byte aligned (`xvec`, `wvec`, decided on the host);
// otherwise every half is loaded on its own, guarded on its own.
#pragma once

namespace {

typedef _Float16 half_t;
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

constexpr int kHalfPitch = KC + 8;  // halves between rows of the LDS images
static_assert(KC == 16, "k_subm_gemm_h: a slice is four 4-half units per row and one MFMA deep");

__device__ __forceinline__ mfma_f32x4 mfma_h(h4 a, h4 b, mfma_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
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
  constexpr int WT = TM * TN == 32 * 32 ? 16 : 32;  // a wave's outputs: WT x WT
  constexpr int FR = WT / 16;                       // 16 x 16 fragments per side
  constexpr int WCOLS = TN / WT;
  static_assert((TM / WT) * WCOLS == 4, "four waves cover the tile");
  constexpr int UA = TM * KC / 4, UB = TN * KC / 4;  // staged units of four halves
  constexpr int NA = (UA + 255) / 256, NB = (UB + 255) / 256;
  constexpr int P = kHalfPitch;
  __shared__ __attribute__((aligned(8))) half_t As[TM * P];
  __shared__ __attribute__((aligned(8))) half_t Bs[TN * P];
  __shared__ int32_t sN[TM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave / WCOLS) * WT, wc = (wave % WCOLS) * WT;
  const int fl = lane & 15, fk = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;
  const int kbeg = blockIdx.z * per, kend = kbeg + per < K ? kbeg + per : K;
  mfma_f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int j = 0; j < FR; j++) acc[i][j] = mfma_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int k = kbeg; k < kend; k++) {
    const int kn = mirror ? K - 1 - k : k;
    int any = 0;
    for (int r = tid; r < TM; r += 256) {
      const int64_t row = row0 + r;
      const int32_t j = row < n ? nbr[row * K + kn] : -1;
      sN[r] = j;
      any |= j >= 0;
    }
    if (!__syncthreads_or(any)) continue;
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
      h4 a[FR], b[FR];
#pragma unroll
      for (int i = 0; i < FR; i++) a[i] = *reinterpret_cast<const h4*>(&As[(wr + 16 * i + fl) * P + 4 * fk]);
#pragma unroll
      for (int j = 0; j < FR; j++) b[j] = *reinterpret_cast<const h4*>(&Bs[(wc + 16 * j + fl) * P + 4 * fk]);
#pragma unroll
      for (int i = 0; i < FR; i++)
#pragma unroll
        for (int j = 0; j < FR; j++) acc[i][j] = mfma_h(a[i], b[j], acc[i][j]);
      __syncthreads();
    }
  }
  float* pdst = part ? part + (int64_t)blockIdx.z * n * nout : nullptr;
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int64_t row = row0 + wr + 16 * i + 4 * fk + v;
      if (row >= n) continue;
      const bool zero = !part && rowmask && rowmask[row] != (int32_t)row;
#pragma unroll
      for (int j = 0; j < FR; j++) {
        const int o = n0 + wc + 16 * j + fl;
        if (o >= nout) continue;
        const float s = acc[i][j][v];
        if (part)
          pdst[row * nout + o] = s;
        else
          y[row * nout + o] = (half_t)(zero ? 0.0f : (bias ? s + (float)bias[o] : s));
      }
    }
}

// out[row][o] = binary16((sum of part[s][row][o], s ascending) + bias[o]); 0 where rowmask[row] != row
__global__ void k_slice_epilogue_h(const float* __restrict__ part, int nslice, int64_t n, int nout,
                                   const half_t* __restrict__ bias, const int32_t* __restrict__ rowmask,
                                   half_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, len = n * nout;
  if (e >= len) return;
  const int64_t row = e / nout;
  const int o = (int)(e - row * nout);
  float v = part[e];
  for (int s = 1; s < nslice; s++) v += part[(int64_t)s * len + e];
  const bool zero = rowmask && rowmask[row] != (int32_t)row;
  out[e] = (half_t)(zero ? 0.0f : (bias ? v + (float)bias[o] : v));
}

bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// launch_gemm_mfma for binary16; `part` is fp32 [S][n][nout] when S > 1.  `wrow` is W's innermost extent (the real cin).
template <bool TRANS>
void launch_gemm_h(int tile, int S, const half_t* x, int cin, const half_t* w, int64_t sk, int64_t sn, int64_t sc, int wrow,
                   const half_t* bias, const int32_t* nbr, int K, int mirror, const int32_t* rowmask, half_t* y, int nout,
                   int64_t n, float* part, hipStream_t st) {
  const int per = (K + S - 1) / S;
  float* p = S > 1 ? part : nullptr;
  const int xvec = cin % 4 == 0 && aligned8(x), wvec = wrow % 4 == 0 && aligned8(w);
  if (tile == GCS_TILE_64X64) {
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)((nout + 63) / 64), (unsigned)S);
    k_subm_gemm_h<64, 64, TRANS><<<grid, 256, 0, st>>>(x, cin, xvec, w, sk, sn, sc, wvec, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  } else if (tile == GCS_TILE_128X32) {
    dim3 grid((unsigned)((n + 127) / 128), 1, (unsigned)S);  // nout <= 32: one column tile
    k_subm_gemm_h<128, 32, TRANS><<<grid, 256, 0, st>>>(x, cin, xvec, w, sk, sn, sc, wvec, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  } else {
    dim3 grid((unsigned)((n + 31) / 32), (unsigned)((nout + 31) / 32), (unsigned)S);
    k_subm_gemm_h<32, 32, TRANS><<<grid, 256, 0, st>>>(x, cin, xvec, w, sk, sn, sc, wvec, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  }
  if (S > 1) {
    const int64_t len = n * nout;
    k_slice_epilogue_h<<<(unsigned)((len + 255) / 256), 256, 0, st>>>(part, S, n, nout, bias, rowmask, y);
  }
}

// ---- dW -------------------------------------------------------------------------------------------------------------
// k_subm_dw_mfma with binary16 operands: the grid, the slices [p0, p1), the zero-filled last chunk and the three loads
// that run ahead are its own; a 16-pair chunk is ONE MFMA per accumulator.  A[row = o][k = pair] and B[k = pair][col = c]
// both want four consecutive PAIRS of one channel on a lane, so the pair-major gathers of dy and x (a thread loads along
// the channels, coalesced) are written to LDS transposed, Dt[o][pair] and Xt[c][pair] at the pitch of 24 halves.  The
// loads are single halves: every row stride and base is accepted.  With one slice the value is rounded to binary16 and
// stored to dw; otherwise the fp32 partial goes to part[s] and k_sum_slices_h rounds after the sum over the slices.
template <int T>
__global__ __launch_bounds__(256) void k_subm_dw_h(const half_t* __restrict__ dy, int cout, const half_t* __restrict__ x,
                                                   int cin, const int32_t* __restrict__ nbr, int K,
                                                   const int32_t* __restrict__ prow, const int32_t* __restrict__ hdr,
                                                   int64_t n, int nslice, float* __restrict__ part,
                                                   half_t* __restrict__ dw) {
  static_assert(T == 32 || T == 64, "tile shape: one staging map serves both images");
  constexpr int WT = T / 2, FR = WT / 16;  // waves 2 x 2, a wave's outputs WT x WT
  constexpr int NQ = KR * T / 256, RSTEP = 256 / T;
  constexpr int P = kHalfPitch;
  static_assert(KR == 16, "a chunk is one MFMA deep");
  __shared__ __attribute__((aligned(8))) half_t Dt[T * P];
  __shared__ __attribute__((aligned(8))) half_t Xt[T * P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * WT, wc = (wave & 1) * WT;
  const int fl = lane & 15, fk = lane >> 4;
  const int sr = tid / T, scol = tid % T;  // staging: pair sr + RSTEP * q, column scol
  const int tiles_c = (cin + T - 1) / T;
  const int o0 = (blockIdx.x / tiles_c) * T, c0 = (blockIdx.x % tiles_c) * T;
  const int k = blockIdx.y, s = blockIdx.z;
  const int64_t cnt = hdr[4 + k];
  const int64_t per = (cnt + nslice - 1) / nslice;
  const int64_t p0 = s * per, p1 = p0 + per < cnt ? p0 + per : cnt;
  mfma_f32x4 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int j = 0; j < FR; j++) acc[i][j] = mfma_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  int32_t ia[NQ], ja[NQ], ib[NQ];  // (row, neighbour) of the chunk after this one; rows of the one after that
  half_t rd[NQ], rx[NQ];
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
      rd[q] = (ia[q] >= 0 && o0 + scol < cout) ? dy[(int64_t)ia[q] * cout + o0 + scol] : (half_t)0.0f;
      rx[q] = (ja[q] >= 0 && c0 + scol < cin) ? x[(int64_t)ja[q] * cin + c0 + scol] : (half_t)0.0f;
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
      Dt[scol * P + sr + RSTEP * q] = rd[q];
      Xt[scol * P + sr + RSTEP * q] = rx[q];
    }
    __syncthreads();
    fetch();
    nbrs(ib, ja);
#pragma unroll
    for (int q = 0; q < NQ; q++) ia[q] = ib[q];
    rows(p + 3 * KR, ib);
    h4 a[FR], b[FR];
#pragma unroll
    for (int i = 0; i < FR; i++) a[i] = *reinterpret_cast<const h4*>(&Dt[(wr + 16 * i + fl) * P + 4 * fk]);
#pragma unroll
    for (int j = 0; j < FR; j++) b[j] = *reinterpret_cast<const h4*>(&Xt[(wc + 16 * j + fl) * P + 4 * fk]);
#pragma unroll
    for (int i = 0; i < FR; i++)
#pragma unroll
      for (int j = 0; j < FR; j++) acc[i][j] = mfma_h(a[i], b[j], acc[i][j]);
    __syncthreads();
  }
  float* out = part ? part + (int64_t)s * cout * K * cin : nullptr;
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int o = o0 + wr + 16 * i + 4 * fk + v;
      if (o >= cout) continue;
#pragma unroll
      for (int j = 0; j < FR; j++) {
        const int c = c0 + wc + 16 * j + fl;
        if (c >= cin) continue;
        const int64_t at = ((int64_t)o * K + k) * cin + c;
        if (part)
          out[at] = acc[i][j][v];
        else
          dw[at] = (half_t)acc[i][j][v];
      }
    }
}

// the launch of k_subm_dw_h: `part` is fp32 [S][cout][K][cin] when S > 1, else dw receives the rounded values
void launch_dw_h(int tile, int S, const half_t* dy, int cout, const half_t* x, int cin, const int32_t* nbr, int K,
                 const int32_t* prow, const int32_t* hdr, int64_t n, float* part, half_t* dw, hipStream_t st) {
  float* p = S > 1 ? part : nullptr;
  if (tile == GCS_TILE_64X64) {
    dim3 grid((unsigned)(((cout + 63) / 64) * ((cin + 63) / 64)), (unsigned)K, (unsigned)S);
    k_subm_dw_h<64><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S, p, dw);
  } else {
    dim3 grid((unsigned)(((cout + 31) / 32) * ((cin + 31) / 32)), (unsigned)K, (unsigned)S);
    k_subm_dw_h<32><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S, p, dw);
  }
}

// ---- the binary16 variants of k_sum_slices, k_colsum and k_fold: fp32 sums in the same fixed order, one rounding -----
__global__ void k_sum_slices_h(const float* __restrict__ part, int nslice, int64_t len, half_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  float v = part[e];
  for (int s = 1; s < nslice; s++) v += part[(int64_t)s * len + e];
  out[e] = (half_t)v;
}

__global__ __launch_bounds__(256) void k_colsum_h(const half_t* __restrict__ dy, int64_t n, int cout, int nslice,
                                                  float* __restrict__ part) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + threadIdx.x % 64, ph = threadIdx.x / 64, s = blockIdx.y;
  const int64_t per = (n + nslice - 1) / nslice, r0 = s * per, r1 = r0 + per < n ? r0 + per : n;
  float v = 0.0f;
  if (col < cout)
    for (int64_t r = r0 + ph; r < r1; r += 4) v += (float)dy[r * cout + col];
  red[ph][threadIdx.x % 64] = v;
  __syncthreads();
  if (ph == 0 && col < cout) part[(int64_t)s * cout + col] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// dyf[r] = binary16(fp32 sum of dy over the rows of representative r's voxel, row order); other rows are never read
__global__ void k_fold_h(const half_t* __restrict__ dy, int64_t n, int cout, const int32_t* __restrict__ rep,
                         const int32_t* __restrict__ gstart, const int32_t* __restrict__ gcnt,
                         const int32_t* __restrict__ glist, half_t* __restrict__ dyf) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cout) return;
  const int64_t r = e / cout;
  const int o = (int)(e - r * cout);
  if (rep[r] != (int32_t)r) return;
  const int cnt = gcnt[r];
  if (cnt < 2) {
    dyf[e] = dy[e];
    return;
  }
  const int32_t* g = glist + gstart[r];
  float v = (float)dy[(int64_t)g[0] * cout + o];
  for (int q = 1; q < cnt; q++) v += (float)dy[(int64_t)g[q] * cout + o];
  dyf[e] = (half_t)v;
}

// ---- segment_csr: k_seg_fwd / k_seg_bwd on binary16 -- fp32 sums in row order, mean divided in fp32, one rounding; min
// and max compare exactly and copy bits ------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_seg_fwd_h(const half_t* __restrict__ src, int64_t m, int64_t f,
                                                  const int64_t* __restrict__ indptr, int64_t nfb, int reduce,
                                                  half_t* __restrict__ out, int64_t* __restrict__ arg) {
  const int64_t s = blockIdx.x / nfb, col = (blockIdx.x % nfb) * 64 + threadIdx.x;
  if (col >= f) return;
  int64_t lo, hi;
  seg_bounds(indptr, s, m, &lo, &hi);
  half_t res = (half_t)0.0f;
  int64_t best = -1;
  if (reduce == GCS_SUM || reduce == GCS_MEAN) {
    float v = 0.0f;
    for (int64_t r = lo; r < hi; r++) v += (float)src[r * f + col];
    if (reduce == GCS_MEAN && hi > lo) v = v / (float)(hi - lo);
    res = (half_t)v;
  } else if (hi > lo) {
    res = src[lo * f + col];
    best = lo;
    for (int64_t r = lo + 1; r < hi; r++) {
      const half_t u = src[r * f + col];
      if (reduce == GCS_MAX ? (float)u > (float)res : (float)u < (float)res) {
        res = u;
        best = r;
      }
    }
  }
  out[s * f + col] = res;
  if (arg) arg[s * f + col] = best;
}

__global__ __launch_bounds__(64) void k_seg_bwd_h(const half_t* __restrict__ dout, int64_t m, int64_t f,
                                                  const int64_t* __restrict__ indptr, int64_t nfb, int reduce,
                                                  const int64_t* __restrict__ arg, half_t* __restrict__ dsrc) {
  const int64_t s = blockIdx.x / nfb, col = (blockIdx.x % nfb) * 64 + threadIdx.x;
  if (col >= f) return;
  int64_t lo, hi;
  seg_bounds(indptr, s, m, &lo, &hi);
  half_t g = dout[s * f + col];
  if (reduce == GCS_MEAN && hi > lo) g = (half_t)((float)g / (float)(hi - lo));
  const int64_t a = (reduce == GCS_MIN || reduce == GCS_MAX) ? arg[s * f + col] : -1;
  for (int64_t r = lo; r < hi; r++)
    dsrc[r * f + col] = (reduce == GCS_SUM || reduce == GCS_MEAN) ? g : (r == a ? g : (half_t)0.0f);
}

}  // namespace
