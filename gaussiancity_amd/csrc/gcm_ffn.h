// gcm_ffn.h -- the feed-forward third of a PTv3 Block (gcm_ffn_*, include/gcm.h): y = x + s o (GELU(LN(x) W1^T + b1) W2^T + b2)
// in ONE launch, and its deterministic backward in a handful of launches whatever N is.  Included by gcm_modlinear.hip,
// whose WaveTile, kPitch / kPitchT images and fetch-ahead it uses; device code and launch helpers only, the C ABI stays
// in gcm_modlinear.hip.  DESIGN.md section 18.
//
// A workgroup (256 threads, 4 waves as 2 x 2) owns T = 64 rows.  CT = 32 NJ (NJ = 1, 2, 4) is the channel width a kernel
// instantiation holds; C <= CT, channels beyond C and rows beyond N are staged as zeros, the summed index over the
// channels runs to C rounded up to 16 only.
//   forward   x tile -> LDS, normalised in place (4 lanes per row, fixed order).  Per chunk of 64 hidden features:
//             a = xn W1^T (one chain over C) + b1 -> stored when the caller asks -> g = GELU(a) in registers -> LDS;
//             t_chunk = g W2^T (one chain over the chunk's 64 features), y accumulators += t_chunk.  The end adds b2,
//             multiplies by s_r, adds x and stores.  A wave's y tile is 32 rows x 16 NJ channels.
//   backward  k_ffn_bwd_rows: dt = s o dy -> LDS; per chunk dg = dt W2 (chain over C), da = dg o gelu'(a) -> workspace
//             and LDS, dxn accumulators += da W1 (chain over the chunk); then dxn -> LDS, the LayerNorm backward per row,
//             dx = dy + ..., and the tile's column sums of dxn o xhat and dxn (row groups in ascending order).
//             k_ffn_dw: dW1 = da^T xn and dW2 = dt^T GELU(a) in row slices (k_modlinear_dw's scheme, both in one
//             launch), with db1 / db2 as the column sums of the slice's da / dt.  k_ffn_fold_params adds the slices
//             pairwise, a fixed tree; k_ffn_fold_groups / k_ffn_fold_ln add the tiles' LayerNorm partials in tile order.
// Nothing depends on how many workgroups are resident: every sum has a fixed set of terms in a fixed order.
#pragma once

namespace {

constexpr int FH = 64;                 // hidden features per chunk
constexpr int kPitchG = FH + 4;        // words between rows of the g / da chunk image (rows x hidden)
constexpr int kFfnMaxChannels = 128;   // widest instantiation (NJ = 4)
constexpr int kFfnFoldTiles = 64;      // LayerNorm partials: up to this many tiles fold in one level
constexpr int kFfnSumRows = 32;        // weight gradients: a chain runs over this many rows, the chains' results are added in order
constexpr int kFfnMaxSlices = 64;      // weight gradients: at most this many row slices, the leaves of k_ffn_fold_params' tree

__device__ __forceinline__ float gelu_f(float a) { return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f)); }
// d/da of gelu: Phi(a) + a phi(a)
__device__ __forceinline__ float gelu_grad_f(float a) {
  const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752f));
  const float pdf = 0.3989422804014327f * expf(-0.5f * a * a);
  return cdf + a * pdf;
}
__device__ __forceinline__ float sum4(float acc, f4 v) {  // one chain, element order
  acc += v[0];
  acc += v[1];
  acc += v[2];
  acc += v[3];
  return acc;
}
__device__ __forceinline__ float quad_sum(float v) {  // the 4 lanes of a row: the same bits in all four
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_ffn_forward(const float* __restrict__ x, int64_t xs, const float* __restrict__ lnw,
                                                        const float* __restrict__ lnb, float eps, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, const float* __restrict__ s, int64_t N,
                                                        int C, int Hd, float* __restrict__ y, int64_t ys,
                                                        float* __restrict__ mean, float* __restrict__ rstd,
                                                        float* __restrict__ a) {
  constexpr int CT = 32 * NJ, XP = CT + 4, NV = NJ > 2 ? NJ / 2 : 1;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];                    // x, then LN(x): rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];               // GELU(a) of one chunk: rows x hidden
  __shared__ __attribute__((aligned(16))) float Ws[(CT > T ? CT : T) * kPitch];  // a 16-deep slice of W1, then of W2
  const int tid = threadIdx.x;
  const WaveTile g;
  const int wcn = (g.wc >> 5) * 16 * NJ;  // the wave's first y channel
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC, c4 = Cr >> 2;

  for (int e = tid; e < T * c4; e += 256) {
    const int r = e / c4, c = 4 * (e % c4);
    *reinterpret_cast<f4*>(&Xs[r * XP + c]) = (row0 + r < N && c < C) ? ld4(x + (row0 + r) * xs + c) : zero4();
  }
  __syncthreads();
  {  // LayerNorm in place: lane q of a row owns the elements 4 q + 16 k .. + 3
    const int r = tid >> 2, q = tid & 3;
    const bool live = row0 + r < N;
    float sum = 0.0f;
    for (int c = 4 * q; c < C; c += 16) sum = sum4(sum, *reinterpret_cast<const f4*>(&Xs[r * XP + c]));
    const float mu = quad_sum(sum) / (float)C;
    float sq = 0.0f;
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu;
      sq = sum4(sq, d * d);
    }
    const float rs = 1.0f / sqrtf(quad_sum(sq) / (float)C + eps);
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu;
      *reinterpret_cast<f4*>(&Xs[r * XP + c]) = live ? d * rs * ld4(lnw + c) + ld4(lnb + c) : zero4();
    }
    if (live && q == 0 && mean) {
      mean[row0 + r] = mu;
      rstd[row0 + r] = rs;
    }
  }
  // (the first __syncthreads of the slice loop below orders these writes before the fragment reads)

  const int br = tid >> 2, bc = 4 * (tid & 3);  // W1 slice: hidden row tid / 4, four channels at 4 * (tid % 4)
  f4 vb, vw[NV];
  auto fetch1 = [&](int h0, int c0) {
    const int h = h0 + br, c = c0 + bc;
    vb = (h < Hd && c < C) ? ld4(w1 + (int64_t)h * C + c) : zero4();
  };
  auto fetch2 = [&](int h0, int k0) {  // W2 slice: channel row e / 4, four hidden features at 4 * (e % 4)
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u, c = e >> 2, h = h0 + k0 + 4 * (e & 3);
      vw[u] = (e < 4 * CT && c < C && h < Hd) ? ld4(w2 + (int64_t)c * Hd + h) : zero4();
    }
  };

  f4 yacc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) yacc[i][j] = zero4();

  for (int h0 = 0; h0 < Hd; h0 += FH) {
    f4 acc[2][2];
    clear_acc(acc);
    fetch1(h0, 0);
    for (int c0 = 0; c0 < Cr; c0 += KC) {
      *reinterpret_cast<f4*>(&Ws[br * kPitch + bc]) = vb;
      __syncthreads();
      if (c0 + KC < Cr) fetch1(h0, c0 + KC);
      else fetch2(h0, 0);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = Xs[(g.wr + 16 * i + g.fl) * XP + c0 + kk + g.fk];
#pragma unroll
        for (int j = 0; j < 2; j++) fb[j] = Ws[(g.wc + 16 * j + g.fl) * kPitch + kk + g.fk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int rl = g.wr + 16 * i + 4 * g.fk + v;
        const int64_t row = row0 + rl;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int hl = g.wc + 16 * j + g.fl, h = h0 + hl;
          float gv = 0.0f;
          if (h < Hd) {
            const float av = acc[i][j][v] + b1[h];
            if (a && row < N) a[row * Hd + h] = av;
            gv = gelu_f(av);
          }
          Gs[rl * kPitchG + hl] = gv;
        }
      }
    const int kend = Hd - h0 < FH ? (Hd - h0 + KC - 1) / KC * KC : FH;
    f4 tacc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) tacc[i][j] = zero4();
    for (int k0 = 0; k0 < kend; k0 += KC) {
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int e = tid + 256 * u;
        if (e < 4 * CT) *reinterpret_cast<f4*>(&Ws[(e >> 2) * kPitch + 4 * (e & 3)]) = vw[u];
      }
      __syncthreads();
      if (k0 + KC < kend) fetch2(h0, k0 + KC);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[NJ];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = Gs[(g.wr + 16 * i + g.fl) * kPitchG + k0 + kk + g.fk];
#pragma unroll
        for (int j = 0; j < NJ; j++) fb[j] = Ws[(wcn + 16 * j + g.fl) * kPitch + kk + g.fk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < NJ; j++) tacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], tacc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) yacc[i][j] = yacc[i][j] + tacc[i][j];
  }

#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int64_t row = row0 + g.wr + 16 * i + 4 * g.fk + v;
      if (row >= N) continue;
      const float sr = s ? s[row] : 1.0f;
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int c = wcn + 16 * j + g.fl;
        if (c >= C) continue;
        const float t = yacc[i][j][v] + b2[c];
        y[row * ys + c] = x[row * xs + c] + (s ? sr * t : t);
      }
    }
}

// ---- backward, the row tiles --------------------------------------------------------------------------------------------
// da [N][Hd] is always written; dx and lnpart [tiles][2][C] (column sums of dxn o xhat, then of dxn) when not null.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_ffn_bwd_rows(const float* __restrict__ x, int64_t xs, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ a,
                                                         const float* __restrict__ dy, int64_t dys, const float* __restrict__ s,
                                                         const float* __restrict__ lnw, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, int64_t N, int C, int Hd,
                                                         float* __restrict__ dx, int64_t dxs, float* __restrict__ da,
                                                         float* __restrict__ lnpart) {
  constexpr int CT = 32 * NJ, XP = CT + 4, WP = CT + 16, NV = NJ > 2 ? NJ / 2 : 1;
  constexpr int CQ = CT / 4, GROUPS = 256 / CQ, RPG = T / GROUPS;  // column sums: f4 columns, row groups, rows per group
  static_assert(GROUPS * 2 * CT <= T * kPitchG, "the column partials live in the chunk image");
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];                    // dt, then dxn: rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];               // da of one chunk; then the column partials
  __shared__ __attribute__((aligned(16))) float Ws[KC * ((CT > T ? CT : T) + 16)];  // a slice of W2 (kPitchT), then of W1 (WP)
  __shared__ float sMean[T], sRstd[T];
  const int tid = threadIdx.x;
  const WaveTile g;
  const int wcn = (g.wc >> 5) * 16 * NJ;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC, c4 = Cr >> 2;

  if (tid < T) {
    const bool live = row0 + tid < N;
    sMean[tid] = live ? mean[row0 + tid] : 0.0f;
    sRstd[tid] = live ? rstd[row0 + tid] : 0.0f;
  }
  for (int e = tid; e < T * c4; e += 256) {
    const int r = e / c4, c = 4 * (e % c4);
    f4 v = zero4();
    if (row0 + r < N && c < C) {
      v = ld4(dy + (row0 + r) * dys + c);
      if (s) v = v * s[row0 + r];
    }
    *reinterpret_cast<f4*>(&Ds[r * XP + c]) = v;
  }
  // (ordered before the fragment reads by the first __syncthreads of the slice loop)

  const int br = tid >> 4, bc = 4 * (tid & 15);  // W2 slice: channel row tid / 16, four hidden features at 4 * (tid % 16)
  f4 vb, vw[NV];
  auto fetch2 = [&](int h0, int c0) {
    const int c = c0 + br, h = h0 + bc;
    vb = (c < C && h < Hd) ? ld4(w2 + (int64_t)c * Hd + h) : zero4();
  };
  auto fetch1 = [&](int h0, int k0) {  // W1 slice: hidden row e / CQ, four channels at 4 * (e % CQ)
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u, h = h0 + k0 + e / CQ, c = 4 * (e % CQ);
      vw[u] = (e < KC * CQ && h < Hd && c < C) ? ld4(w1 + (int64_t)h * C + c) : zero4();
    }
  };

  f4 xacc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) xacc[i][j] = zero4();

  for (int h0 = 0; h0 < Hd; h0 += FH) {
    f4 acc[2][2];
    clear_acc(acc);
    fetch2(h0, 0);
    for (int c0 = 0; c0 < Cr; c0 += KC) {
      *reinterpret_cast<f4*>(&Ws[br * kPitchT + bc]) = vb;
      __syncthreads();
      if (c0 + KC < Cr) fetch2(h0, c0 + KC);
      else fetch1(h0, 0);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = Ds[(g.wr + 16 * i + g.fl) * XP + c0 + kk + g.fk];
#pragma unroll
        for (int j = 0; j < 2; j++) fb[j] = Ws[(kk + g.fk) * kPitchT + g.wc + 16 * j + g.fl];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int rl = g.wr + 16 * i + 4 * g.fk + v;
        const int64_t row = row0 + rl;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int hl = g.wc + 16 * j + g.fl, h = h0 + hl;
          float dv = 0.0f;
          if (h < Hd && row < N) {
            dv = acc[i][j][v] * gelu_grad_f(a[row * Hd + h]);
            da[row * Hd + h] = dv;
          }
          Gs[rl * kPitchG + hl] = dv;
        }
      }
    const int kend = Hd - h0 < FH ? (Hd - h0 + KC - 1) / KC * KC : FH;
    f4 tacc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) tacc[i][j] = zero4();
    for (int k0 = 0; k0 < kend; k0 += KC) {
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int e = tid + 256 * u;
        if (e < KC * CQ) *reinterpret_cast<f4*>(&Ws[(e / CQ) * WP + 4 * (e % CQ)]) = vw[u];
      }
      __syncthreads();
      if (k0 + KC < kend) fetch1(h0, k0 + KC);
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[NJ];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = Gs[(g.wr + 16 * i + g.fl) * kPitchG + k0 + kk + g.fk];
#pragma unroll
        for (int j = 0; j < NJ; j++) fb[j] = Ws[(kk + g.fk) * WP + wcn + 16 * j + g.fl];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < NJ; j++) tacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], tacc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) xacc[i][j] = xacc[i][j] + tacc[i][j];
  }

  // dxn over dt's image (its last fragment read is behind the __syncthreads that closed the last chain over C)
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int rl = g.wr + 16 * i + 4 * g.fk + v;
#pragma unroll
      for (int j = 0; j < NJ; j++) Ds[rl * XP + wcn + 16 * j + g.fl] = xacc[i][j][v];
    }
  __syncthreads();

  if (dx) {  // LayerNorm backward: lane q of a row owns the elements 4 q + 16 k .. + 3
    const int r = tid >> 2, q = tid & 3;
    const int64_t row = row0 + r;
    const bool live = row < N;
    const float mu = sMean[r], rs = sRstd[r];
    f4 xh[2 * NJ], wd[2 * NJ];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      xh[k] = zero4();
      wd[k] = zero4();
      if (live && c < C) {
        xh[k] = (ld4(x + row * xs + c) - mu) * rs;
        wd[k] = *reinterpret_cast<const f4*>(&Ds[r * XP + c]) * ld4(lnw + c);
        s1 = sum4(s1, wd[k]);
        s2 = sum4(s2, wd[k] * xh[k]);
      }
    }
    const float c1 = quad_sum(s1) / (float)C, c2 = quad_sum(s2) / (float)C;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      if (live && c < C)
        *reinterpret_cast<f4*>(dx + row * dxs + c) = ld4(dy + row * dys + c) + (wd[k] - c1 - xh[k] * c2) * rs;
    }
  }
  if (!lnpart) return;

  {  // the tile's column sums: thread (row group, f4 column) sums its RPG rows in order, then the groups in order
    const int cq = tid % CQ, grp = tid / CQ, c = 4 * cq;
    f4 pg = zero4(), pb = zero4();
    if (c < C) {
#pragma unroll
      for (int k = 0; k < RPG; k++) {
        const int r = grp * RPG + k;
        if (row0 + r >= N) break;
        const f4 d = *reinterpret_cast<const f4*>(&Ds[r * XP + c]);
        const f4 h = (ld4(x + (row0 + r) * xs + c) - sMean[r]) * sRstd[r];
        pg = pg + d * h;
        pb = pb + d;
      }
    }
    *reinterpret_cast<f4*>(&Gs[(grp * 2 + 0) * CT + c]) = pg;
    *reinterpret_cast<f4*>(&Gs[(grp * 2 + 1) * CT + c]) = pb;
  }
  __syncthreads();
  if (tid < 2 * CT) {
    const int which = tid / CT, c = tid % CT;
    if (c < C) {
      float v = Gs[which * CT + c];
      for (int grp = 1; grp < GROUPS; grp++) v += Gs[(grp * 2 + which) * CT + c];
      lnpart[((int64_t)blockIdx.x * 2 + which) * C + c] = v;
    }
  }
}

// ---- backward, the two weight gradients ---------------------------------------------------------------------------------
// A slice's record in `part`: dW1 [Hd][C], dW2 [C][Hd], db1 [Hd], db2 [C].
__host__ __device__ inline int64_t ffn_record(int C, int Hd) { return 2 * (int64_t)C * Hd + Hd + C; }

// One 64 x 64 tile of a row-sliced weight gradient and its bias gradient, shared by k_ffn_dw and k_front_dw (gcm_front.h):
// dst[o][i] = sum_r d[r][o] x[r][i] (row pitch I) and, from the tiles with i0 == 0, bias[o] = sum_r d[r][o], over the rows
// p0 .. p1 in ascending order.  fetch(r, od, ix, vd, vx) loads row r's four "d" elements at o0 + sc (when od) and four "x"
// elements at i0 + sc (when ix); Od, I: the extents of the two operands.  One chain from 0 per kFfnSumRows rows, those sums
// added in ascending order (shorter chains: the rounding grows with the root of the chain's length).
template <typename Fetch>
__device__ __forceinline__ void dw_slice_tile(Fetch fetch_row, int Od, int I, int o0, int i0, int64_t p0, int64_t p1,
                                              float* __restrict__ dst, float* __restrict__ bias, float* Ds, float* Xs) {
  const int tid = threadIdx.x;
  const WaveTile g;
  const int sp = tid >> 4, sc = 4 * (tid & 15);
  const bool od = o0 + sc < Od, ix = i0 + sc < I;
  f4 vd, vx;
  auto fetch = [&](int64_t p) {
    vd = zero4();
    vx = zero4();
    if (p + sp < p1) fetch_row(p + sp, od, ix, vd, vx);
  };
  f4 acc[2][2], tot[2][2];  // acc: the chain over the current kFfnSumRows rows; tot: those sums, ascending
  clear_acc(acc);
  clear_acc(tot);
  float bsum = 0.0f, btot = 0.0f;
  auto flush = [&]() {
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        tot[i][j] = tot[i][j] + acc[i][j];
        acc[i][j] = zero4();
      }
    btot += bsum;
    bsum = 0.0f;
  };
  fetch(p0);
  for (int64_t p = p0; p < p1; p += KC) {
    if (p != p0 && (p - p0) % kFfnSumRows == 0) flush();
    *reinterpret_cast<f4*>(&Ds[sp * kPitchT + sc]) = vd;
    *reinterpret_cast<f4*>(&Xs[sp * kPitchT + sc]) = vx;
    __syncthreads();
    if (p + KC < p1) fetch(p + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      float fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; i++) fa[i] = Ds[(kk + g.fk) * kPitchT + g.wr + 16 * i + g.fl];
#pragma unroll
      for (int j = 0; j < 2; j++) fb[j] = Xs[(kk + g.fk) * kPitchT + g.wc + 16 * j + g.fl];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (i0 == 0 && tid < T) {  // the bias gradient: the column sums of the "d" operand, four chains of four rows, paired
      float q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        q[k] = Ds[4 * k * kPitchT + tid];
#pragma unroll
        for (int m = 1; m < 4; m++) q[k] += Ds[(4 * k + m) * kPitchT + tid];
      }
      bsum += (q[0] + q[1]) + (q[2] + q[3]);
    }
    __syncthreads();
  }
  flush();
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int o = o0 + g.wr + 16 * i + 4 * g.fk + v;
      if (o >= Od) continue;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int c = i0 + g.wc + 16 * j + g.fl;
        if (c < I) dst[(int64_t)o * I + c] = tot[i][j][v];
      }
    }
  if (i0 == 0 && tid < T && o0 + tid < Od) bias[o0 + tid] = btot;
}

// MODE 0: dW1[h][c] = sum_r da[r][h] xn[r][c], db1[h] = sum_r da[r][h].   MODE 1: dW2[c][h] = sum_r dt[r][c] g[r][h],
// db2[c] = sum_r dt[r][c].  O, I: the extents of the "d" and the "x" operand.
template <int MODE>
__device__ __forceinline__ void ffn_dw_tile(const float* __restrict__ x, int64_t xs, const float* __restrict__ mean,
                                            const float* __restrict__ rstd, const float* __restrict__ a,
                                            const float* __restrict__ da, const float* __restrict__ dy, int64_t dys,
                                            const float* __restrict__ s, const float* __restrict__ lnw,
                                            const float* __restrict__ lnb, int64_t N, int C, int Hd, int64_t per,
                                            float* __restrict__ rec, float* Ds, float* Xs) {
  const int O = MODE == 0 ? Hd : C, I = MODE == 0 ? C : Hd;
  const int tiles_i = (I + T - 1) / T;
  const int o0 = (blockIdx.x / tiles_i) * T, i0 = (blockIdx.x % tiles_i) * T;
  const int64_t p0 = blockIdx.y * per, p1 = p0 + per < N ? p0 + per : N;
  const int sc = 4 * (threadIdx.x & 15);
  f4 gam = zero4(), bet = zero4();
  if (MODE == 0 && i0 + sc < I) {
    gam = ld4(lnw + i0 + sc);
    bet = ld4(lnb + i0 + sc);
  }
  auto fetch = [&](int64_t r, bool od, bool ix, f4& vd, f4& vx) {
    if (MODE == 0) {
      if (od) vd = ld4(da + r * Hd + o0 + sc);
      if (ix) vx = (ld4(x + r * xs + i0 + sc) - mean[r]) * rstd[r] * gam + bet;
    } else {
      if (od) {
        vd = ld4(dy + r * dys + o0 + sc);
        if (s) vd = vd * s[r];
      }
      if (ix) {
        const f4 av = ld4(a + r * Hd + i0 + sc);
#pragma unroll
        for (int k = 0; k < 4; k++) vx[k] = gelu_f(av[k]);
      }
    }
  };
  const int64_t CH = (int64_t)C * Hd;
  dw_slice_tile(fetch, O, I, o0, i0, p0, p1, rec + (MODE == 0 ? 0 : CH), rec + 2 * CH + (MODE == 0 ? 0 : Hd), Ds, Xs);
}

// grid: (tiles of 64 x 64 over Hd x C, row slices, 2): z = 0 is dW1 / db1, z = 1 is dW2 / db2
__global__ __launch_bounds__(256) void k_ffn_dw(const float* __restrict__ x, int64_t xs, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, const float* __restrict__ a,
                                                const float* __restrict__ da, const float* __restrict__ dy, int64_t dys,
                                                const float* __restrict__ s, const float* __restrict__ lnw,
                                                const float* __restrict__ lnb, int64_t N, int C, int Hd, int64_t per,
                                                float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ds[KC * kPitchT];
  __shared__ __attribute__((aligned(16))) float Xs[KC * kPitchT];
  float* rec = part + (int64_t)blockIdx.y * ffn_record(C, Hd);
  if (blockIdx.z == 0) ffn_dw_tile<0>(x, xs, mean, rstd, a, da, dy, dys, s, lnw, lnb, N, C, Hd, per, rec, Ds, Xs);
  else ffn_dw_tile<1>(x, xs, mean, rstd, a, da, dy, dys, s, lnw, lnb, N, C, Hd, per, rec, Ds, Xs);
}

// the four parameter gradients: the slices' records added pairwise -- one fixed tree over kFfnMaxSlices leaves (level w =
// 1, 2, 4 .. adds slice s + w to slice s; a slice beyond S counts as 0 and x + 0 is x), so the rounding grows with the
// depth of the tree and not with the number of slices: folded as one chain, db2 missed the bar at N = 4097.
// A record is four pieces of n0, n1, n2, n3 elements (ffn_record; front_record of gcm_front.h); a null output is skipped.
__global__ void k_ffn_fold_params(const float* __restrict__ part, int S, int64_t n0, int64_t n1, int64_t n2, int64_t n3,
                                  float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ o2,
                                  float* __restrict__ o3) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, len = n0 + n1 + n2 + n3;
  if (e >= len) return;
  float* out = e < n0 ? (o0 ? o0 + e : nullptr)
               : e < n0 + n1 ? (o1 ? o1 + (e - n0) : nullptr)
               : e < n0 + n1 + n2 ? (o2 ? o2 + (e - n0 - n1) : nullptr) : (o3 ? o3 + (e - n0 - n1 - n2) : nullptr);
  if (!out) return;
  float v[kFfnMaxSlices];
#pragma unroll
  for (int s = 0; s < kFfnMaxSlices; s++) v[s] = s < S ? part[(int64_t)s * len + e] : 0.0f;
#pragma unroll
  for (int w = 1; w < kFfnMaxSlices; w *= 2)
#pragma unroll
    for (int s = 0; s < kFfnMaxSlices; s += 2 * w) v[s] += v[s + w];
  *out = v[0];
}

// out[q][e] = sum of part[s][e] over the `per` records of group q (blockIdx.y), s ascending
__global__ void k_ffn_fold_groups(const float* __restrict__ part, int64_t S, int len, int64_t per, float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  const int64_t s0 = blockIdx.y * per, s1 = s0 + per < S ? s0 + per : S;
  float v = 0.0f;
  for (int64_t s = s0; s < s1; s++) v += part[s * len + e];
  out[(int64_t)blockIdx.y * len + e] = v;
}

// dgamma, dbeta: the records [2][C] in order
__global__ void k_ffn_fold_ln(const float* __restrict__ part, int64_t S, int C, float* __restrict__ dlnw,
                              float* __restrict__ dlnb) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * C) return;
  float* out = e < C ? (dlnw ? dlnw + e : nullptr) : (dlnb ? dlnb + (e - C) : nullptr);
  if (!out) return;
  float v = part[e];
  for (int64_t s = 1; s < S; s++) v += part[s * 2 * C + e];
  *out = v;
}

// ---- host: the plan and the launches ------------------------------------------------------------------------------------
struct FfnPlan {
  int64_t tiles;   // row tiles
  int64_t groups;  // first-level groups of the LayerNorm partials (0: one level)
  int64_t gper;    // tiles per group
  int sw;          // row slices of the weight gradients
  size_t da, lnpart, lngroup, wpart, total;
};
FfnPlan ffn_plan(int64_t N, int32_t C, int32_t Hd) {
  FfnPlan p;
  p.tiles = (N + T - 1) / T;
  p.groups = p.tiles > kFfnFoldTiles ? std::min<int64_t>(256, (p.tiles + kFfnFoldTiles - 1) / kFfnFoldTiles) : 0;
  p.gper = p.groups ? (p.tiles + p.groups - 1) / p.groups : 0;
  const int64_t wt = (int64_t)((Hd + T - 1) / T) * ((C + T - 1) / T);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kFfnMaxSlices, 1024 / wt));
  p.sw = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (N + 63) / 64));
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  p.da = take((size_t)N * Hd * 4);
  p.lnpart = take((size_t)p.tiles * 2 * C * 4);
  p.lngroup = take((size_t)p.groups * 2 * C * 4);
  p.wpart = take((size_t)p.sw * (size_t)ffn_record(C, Hd) * 4);
  p.total = off;
  return p;
}

template <typename... A>
void ffn_launch_forward(int C, dim3 grid, hipStream_t st, A... args) {
  if (C <= 32) k_ffn_forward<1><<<grid, 256, 0, st>>>(args...);
  else if (C <= 64) k_ffn_forward<2><<<grid, 256, 0, st>>>(args...);
  else k_ffn_forward<4><<<grid, 256, 0, st>>>(args...);
}
template <typename... A>
void ffn_launch_bwd_rows(int C, dim3 grid, hipStream_t st, A... args) {
  if (C <= 32) k_ffn_bwd_rows<1><<<grid, 256, 0, st>>>(args...);
  else if (C <= 64) k_ffn_bwd_rows<2><<<grid, 256, 0, st>>>(args...);
  else k_ffn_bwd_rows<4><<<grid, 256, 0, st>>>(args...);
}

}  // namespace
