// gcs_mfma.h -- the matrix-core engine of the submanifold convolution (GCS_ENGINE_MFMA, include/gcs.h): its three products
// on v_mfma_f32_16x16x4_f32.  The gather-GEMM of k_subm_gemm (forward and dX) with the tap slices for grids too small to
// fill the GPU comes first, the weight gradient of k_subm_dw (k_subm_dw_mfma, with its own comment) last.  Included by
// gcs_sparse.hip after k_subm_gemm (it uses KC and KR); device code and launch helpers only, the C ABI stays in
// gcs_sparse.hip.
//
// Forward and dX.  Contract, the same as k_subm_gemm's: every output element is ONE chain from 0.0f over (tap in loop order, channel
// ascending), the bias added after the chain.  The f32-input MFMA is a k-ordered fmaf chain (one rounding per product,
// nothing wider inside), so with the same workgroup tile (gemm_tile), the same block-uniform tap skip and the same
// 16-channel zero-padded slices this kernel gives k_subm_gemm's values; tests/test_sparse_engine_gpu.py holds it to that.
//
// 256 threads = 4 waves.  A wave owns 16 x 16 (32 x 32 tile: waves 2 x 2) or 32 x 32 outputs (64 x 64: waves 2 x 2,
// 128 x 32: waves 4 x 1), that is 1 or 2 x 2 independent accumulators of 4 VGPRs.  Per 16-channel slice four MFMAs per
// accumulator, k = 4 channels each, chained in channel order.  Fragments come from LDS, one VGPR per operand:
//   A  lane l holds A[row l & 15][k = l >> 4]: the gathered rows, As[row][channel], pitch 20 words -- the 64 lanes of a
//      fragment read hit 64 different banks, and so do the 64 lanes of a staging write;
//   B  lane l holds B[k = l >> 4][col l & 15]: forward Bs[col][channel] at pitch 20 (W is read along channels), dX
//      Bs[channel][col] at pitch TN + 16 (W is read along columns): conflict-free both ways in both cases;
//   C  col = lane & 15, row = 4 * (lane >> 4) + reg.
// The global loads of slice c + 1 are issued into registers before the MFMAs of slice c and stored to LDS after them.
//
// Tap slices: grid.z = S, slice s owns taps [s * per, min(K, (s + 1) * per)) of the loop order and, when S > 1, writes
// its partial tile to part[s][n][nout] -- always, zeros included, so what the workspace held before never matters;
// k_slice_epilogue then writes out = (sum of part[s], s ascending) + bias, 0 for the rows the mask excludes.  With
// S == 1 the kernel writes `out` itself, exactly as k_subm_gemm does.
#pragma once

namespace {

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFragPitch = KC + 4;  // words between rows of As (and of the forward's Bs)

template <int TM, int TN, bool TRANS>
__global__ __launch_bounds__(256) void k_subm_gemm_mfma(const float* __restrict__ x, int cin, const float* __restrict__ w,
                                                        int64_t sk, int64_t sn, int64_t sc, const float* __restrict__ bias,
                                                        const int32_t* __restrict__ nbr, int K, int mirror,
                                                        const int32_t* __restrict__ rowmask, float* __restrict__ y, int nout,
                                                        int64_t n, int per, float* __restrict__ part) {
  constexpr int WT = TM * TN == 32 * 32 ? 16 : 32;  // a wave's outputs: WT x WT
  constexpr int FR = WT / 16;                       // 16 x 16 fragments per side
  constexpr int WCOLS = TN / WT;
  static_assert((TM / WT) * WCOLS == 4, "four waves cover the tile");
  constexpr int NA = TM * KC / 256, NB = TN * KC / 256;  // staged elements per thread
  constexpr int BPITCH = TRANS ? TN + 16 : kFragPitch;
  __shared__ float As[TM * kFragPitch];
  __shared__ float Bs[TRANS ? KC * BPITCH : TN * BPITCH];
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
        for (int i = 0; i < FR; i++) a[i] = As[(wr + 16 * i + fl) * kFragPitch + kk + fk];
#pragma unroll
        for (int j = 0; j < FR; j++)
          b[j] = TRANS ? Bs[(kk + fk) * BPITCH + wc + 16 * j + fl] : Bs[(wc + 16 * j + fl) * BPITCH + kk + fk];
#pragma unroll
        for (int i = 0; i < FR; i++)
#pragma unroll
          for (int j = 0; j < FR; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  float* dst = part ? part + (int64_t)blockIdx.z * n * nout : y;
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
        dst[row * nout + o] = part ? s : (zero ? 0.0f : (bias ? s + bias[o] : s));
      }
    }
}

// out[row][o] = (sum of part[s][row][o], s ascending) + bias[o]; 0 where rowmask[row] != row
__global__ void k_slice_epilogue(const float* __restrict__ part, int nslice, int64_t n, int nout,
                                 const float* __restrict__ bias, const int32_t* __restrict__ rowmask,
                                 float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, len = n * nout;
  if (e >= len) return;
  const int64_t row = e / nout;
  const int o = (int)(e - row * nout);
  float v = part[e];
  for (int s = 1; s < nslice; s++) v += part[(int64_t)s * len + e];
  const bool zero = rowmask && rowmask[row] != (int32_t)row;
  out[e] = zero ? 0.0f : (bias ? v + bias[o] : v);
}

// the launch of launch_gemm on the matrix cores, in S tap slices; `part` is [S][n][nout] when S > 1
template <bool TRANS>
void launch_gemm_mfma(int tile, int S, const float* x, int cin, const float* w, int64_t sk, int64_t sn, int64_t sc,
                      const float* bias, const int32_t* nbr, int K, int mirror, const int32_t* rowmask, float* y, int nout,
                      int64_t n, float* part, hipStream_t st) {
  const int per = (K + S - 1) / S;
  float* p = S > 1 ? part : nullptr;
  if (tile == GCS_TILE_64X64) {
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)((nout + 63) / 64), (unsigned)S);
    k_subm_gemm_mfma<64, 64, TRANS><<<grid, 256, 0, st>>>(x, cin, w, sk, sn, sc, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  } else if (tile == GCS_TILE_128X32) {
    dim3 grid((unsigned)((n + 127) / 128), 1, (unsigned)S);  // nout <= 32: one column tile
    k_subm_gemm_mfma<128, 32, TRANS><<<grid, 256, 0, st>>>(x, cin, w, sk, sn, sc, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  } else {
    dim3 grid((unsigned)((n + 31) / 32), (unsigned)((nout + 31) / 32), (unsigned)S);
    k_subm_gemm_mfma<32, 32, TRANS><<<grid, 256, 0, st>>>(x, cin, w, sk, sn, sc, bias, nbr, K, mirror, rowmask, y, nout, n, per, p);
  }
  if (S > 1) {
    const int64_t len = n * nout;
    k_slice_epilogue<<<(unsigned)((len + 255) / 256), 256, 0, st>>>(part, S, n, nout, bias, rowmask, y);
  }
}

// ---- dW -------------------------------------------------------------------------------------------------------------
// k_subm_dw on the matrix cores: part[s][o][k][c] = sum over the pairs p of slice s of tap k: dy[i_p][o] * x[nbr[i_p][k]][c].
// The grid, the slices [p0, p1) and the zero-filled last chunk are k_subm_dw's; every element is one chain from 0.0f over
// the slice's pairs in list order, KR pairs per chunk = four chained MFMAs per accumulator.  Square tiles, T = 64 or 32.
// Both operands are pair-major LDS images at a pitch of T + 16 words, Ds[pair][o] and Xs[pair][c]: the 64 lanes of a
// fragment read (4 pairs x 16 columns) fall on 64 banks (pitch mod 64 = 16 or 48), a staging write is contiguous.
// Three loads run ahead of the MFMAs of chunk c, none depending on another: the rows of x / dy of chunk c + 1, the nbr
// entries of chunk c + 2, the prow entries of chunk c + 3.  A thread stages NQ = T / 16 elements of each image, in the
// pairs r = tid / T + (256 / T) q, and keeps the indices of those pairs itself (a wave asks for one or two addresses).
template <int TO, int TC>
__global__ __launch_bounds__(256) void k_subm_dw_mfma(const float* __restrict__ dy, int cout, const float* __restrict__ x,
                                                      int cin, const int32_t* __restrict__ nbr, int K,
                                                      const int32_t* __restrict__ prow, const int32_t* __restrict__ hdr,
                                                      int64_t n, int nslice, float* __restrict__ part) {
  static_assert(TO == TC && (TO == 32 || TO == 64), "tile shape: one staging map serves both images");
  constexpr int T = TO;
  constexpr int WT = T / 2, FR = WT / 16;  // waves 2 x 2, a wave's outputs WT x WT
  constexpr int NQ = KR * T / 256, RSTEP = 256 / T;
  constexpr int PITCH = T + 16;
  __shared__ float Ds[KR * PITCH];
  __shared__ float Xs[KR * PITCH];
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
  float rd[NQ], rx[NQ];
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
      rd[q] = (ia[q] >= 0 && o0 + scol < cout) ? dy[(int64_t)ia[q] * cout + o0 + scol] : 0.0f;
      rx[q] = (ja[q] >= 0 && c0 + scol < cin) ? x[(int64_t)ja[q] * cin + c0 + scol] : 0.0f;
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
      Ds[(sr + RSTEP * q) * PITCH + scol] = rd[q];
      Xs[(sr + RSTEP * q) * PITCH + scol] = rx[q];
    }
    __syncthreads();
    fetch();
    nbrs(ib, ja);
#pragma unroll
    for (int q = 0; q < NQ; q++) ia[q] = ib[q];
    rows(p + 3 * KR, ib);
#pragma unroll
    for (int kk = 0; kk < KR; kk += 4) {
      float a[FR], b[FR];
#pragma unroll
      for (int i = 0; i < FR; i++) a[i] = Ds[(kk + fk) * PITCH + wr + 16 * i + fl];
#pragma unroll
      for (int j = 0; j < FR; j++) b[j] = Xs[(kk + fk) * PITCH + wc + 16 * j + fl];
#pragma unroll
      for (int i = 0; i < FR; i++)
#pragma unroll
        for (int j = 0; j < FR; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  float* out = part + (int64_t)s * cout * K * cin;
#pragma unroll
  for (int i = 0; i < FR; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int o = o0 + wr + 16 * i + 4 * fk + v;
      if (o >= cout) continue;
#pragma unroll
      for (int j = 0; j < FR; j++) {
        const int c = c0 + wc + 16 * j + fl;
        if (c < cin) out[((int64_t)o * K + k) * cin + c] = acc[i][j][v];
      }
    }
}

// the launch of k_subm_dw on the matrix cores: the same grid, slices and destination
void launch_dw_mfma(int tile, int S, const float* dy, int cout, const float* x, int cin, const int32_t* nbr, int K,
                    const int32_t* prow, const int32_t* hdr, int64_t n, float* dst, hipStream_t st) {
  if (tile == GCS_TILE_64X64) {
    dim3 grid((unsigned)(((cout + 63) / 64) * ((cin + 63) / 64)), (unsigned)K, (unsigned)S);
    k_subm_dw_mfma<64, 64><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S, dst);
  } else {
    dim3 grid((unsigned)(((cout + 31) / 32) * ((cin + 31) / 32)), (unsigned)K, (unsigned)S);
    k_subm_dw_mfma<32, 32><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S, dst);
  }
}

}  // namespace
