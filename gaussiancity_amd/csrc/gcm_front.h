// gcm_front.h -- the front of a PTv3 Block between its sparse convolution and its attention (gcm_front_*, include/gcm.h):
// t = s Wc^T + bc, feat = x + LN_c(t), qkv = LN_1(feat) Wq^T + bq in ONE launch, and its deterministic backward in four
// launches (five beyond 64 row tiles) whatever N is.  Included by gcm_modlinear.hip after gcm_ffn.h, whose tile shape,
// LayerNorm lane rule, chunk image, row-sliced weight gradients and tile-ordered LayerNorm partials it rearranges; device
// code and launch helpers only, the C ABI stays in gcm_modlinear.hip.  DESIGN.md section 19.
//
// A workgroup (256 threads, 4 waves as 2 x 2) owns T = 64 rows; CT = 32 NJ (NJ = 1, 2, 4) is the channel width an
// instantiation holds, C <= CT, channels beyond C and rows beyond N are zeros, the summed index over the channels runs to
// C rounded up to 16 only.
//   forward   s tile -> LDS; t accumulators (a wave's 32 rows x 16 NJ channels, one chain over C) stay in registers until
//             every wave has read s, then t + bc overwrites the tile.  Four lanes per row: LN_c, feat = x + u stored and
//             written back to the tile, LN_1 in place.  qkv per chunk of 64 outputs: one chain over C, + bq, stored.
//   backward  k_front_bwd_rows: per chunk of 64 outputs dqkv -> LDS, dn accumulators += dqkv_chunk Wq (one chain over the
//             chunk); dn -> LDS; the tile's column sums of dn o fhat and dn; LN_1 backward per row with feat read per row,
//             df = dfeat + ..., stored as dx and written back; the column sums of df o that and df; LN_c backward per row
//             with t read per row, dt -> workspace and LDS; ds = dt Wc (one chain over C) from the LDS image.
//             k_front_dw: dWq = dqkv^T n (n rebuilt from feat and LN_1's statistics) and dWc = dt^T s in row slices, both
//             in one launch, with dbq / dbc as the column sums of the slice's dqkv / dt.  k_ffn_fold_params adds the
//             slices pairwise, a fixed tree; k_ffn_fold_groups / k_front_fold_ln add the tiles' partials of BOTH LayerNorms
//             (a record is [4][C]: dg1, dbe1, dgc, dbec) in tile order, one launch per level.
// Nothing depends on how many workgroups are resident: every sum has a fixed set of terms in a fixed order.
#pragma once

namespace {

constexpr int kFrontMaxChannels = kFfnMaxChannels;  // widest instantiation (NJ = 4); O up to three times that

__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }

// ---- forward ----------------------------------------------------------------------------------------------------------
// t, meanc, rstdc, mean1, rstd1: all null (inference) or all stored.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_front_forward(const float* __restrict__ x, int64_t xs, const float* __restrict__ s,
                                                          int64_t ss, const float* __restrict__ wc, const float* __restrict__ bc,
                                                          const float* __restrict__ gc, const float* __restrict__ bec, float epsc,
                                                          const float* __restrict__ g1, const float* __restrict__ be1, float eps1,
                                                          const float* __restrict__ wq, const float* __restrict__ bq, int64_t N,
                                                          int C, int O, float* __restrict__ feat, int64_t fs,
                                                          float* __restrict__ qkv, int64_t qs, float* __restrict__ t,
                                                          float* __restrict__ meanc, float* __restrict__ rstdc,
                                                          float* __restrict__ mean1, float* __restrict__ rstd1) {
  constexpr int CT = 32 * NJ, XP = CT + 4, NV = NJ > 2 ? NJ / 2 : 1;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];                      // s, then t, feat and LN_1(feat): rows x channels
  __shared__ __attribute__((aligned(16))) float Ws[(CT > T ? CT : T) * kPitch];  // a 16-deep slice of Wc, then of Wq
  const int tid = threadIdx.x;
  const WaveTile g;
  const int wcn = (g.wc >> 5) * 16 * NJ;  // the wave's first t channel
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC, c4 = Cr >> 2;

  for (int e = tid; e < T * c4; e += 256) {
    const int r = e / c4, c = 4 * (e % c4);
    *reinterpret_cast<f4*>(&Xs[r * XP + c]) = (row0 + r < N && c < C) ? ld4(s + (row0 + r) * ss + c) : zero4();
  }
  // (ordered before the fragment reads by the first __syncthreads of the slice loop)

  f4 vw[NV];
  auto fetchc = [&](int k0) {  // Wc slice: output channel row e / 4, four input channels at 4 * (e % 4)
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u, c = e >> 2, k = k0 + 4 * (e & 3);
      vw[u] = (e < 4 * CT && c < C && k < C) ? ld4(wc + (int64_t)c * C + k) : zero4();
    }
  };
  f4 tacc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) tacc[i][j] = zero4();
  fetchc(0);
  for (int k0 = 0; k0 < Cr; k0 += KC) {
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u;
      if (e < 4 * CT) *reinterpret_cast<f4*>(&Ws[(e >> 2) * kPitch + 4 * (e & 3)]) = vw[u];
    }
    __syncthreads();
    if (k0 + KC < Cr) fetchc(k0 + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      float fa[2], fb[NJ];
#pragma unroll
      for (int i = 0; i < 2; i++) fa[i] = Xs[(g.wr + 16 * i + g.fl) * XP + k0 + kk + g.fk];
#pragma unroll
      for (int j = 0; j < NJ; j++) fb[j] = Ws[(wcn + 16 * j + g.fl) * kPitch + kk + g.fk];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) tacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], tacc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // every wave is past its last read of s: t + bc over the tile (channels beyond C stay zeros for the chain of qkv)
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int rl = g.wr + 16 * i + 4 * g.fk + v;
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int c = wcn + 16 * j + g.fl;
        Xs[rl * XP + c] = c < C ? tacc[i][j][v] + bc[c] : 0.0f;
      }
    }
  __syncthreads();

  {  // the two LayerNorms in place: lane q of a row owns the elements 4 q + 16 k .. + 3
    const int r = tid >> 2, q = tid & 3;
    const int64_t row = row0 + r;
    const bool live = row < N;
    float sum = 0.0f;
    for (int c = 4 * q; c < C; c += 16) {
      const f4 v = *reinterpret_cast<const f4*>(&Xs[r * XP + c]);
      sum = sum4(sum, v);
      if (t && live) st4(t + row * C + c, v);
    }
    const float mu = quad_sum(sum) / (float)C;
    float sq = 0.0f;
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu;
      sq = sum4(sq, d * d);
    }
    const float rs = 1.0f / sqrtf(quad_sum(sq) / (float)C + epsc);
    float sum1 = 0.0f;
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu;
      f4 f = zero4();
      if (live) {
        f = ld4(x + row * xs + c) + (d * rs * ld4(gc + c) + ld4(bec + c));
        st4(feat + row * fs + c, f);
      }
      *reinterpret_cast<f4*>(&Xs[r * XP + c]) = f;
      sum1 = sum4(sum1, f);
    }
    const float mu1 = quad_sum(sum1) / (float)C;
    float sq1 = 0.0f;
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu1;
      sq1 = sum4(sq1, d * d);
    }
    const float rs1 = 1.0f / sqrtf(quad_sum(sq1) / (float)C + eps1);
    for (int c = 4 * q; c < C; c += 16) {
      const f4 d = *reinterpret_cast<const f4*>(&Xs[r * XP + c]) - mu1;
      *reinterpret_cast<f4*>(&Xs[r * XP + c]) = live ? d * rs1 * ld4(g1 + c) + ld4(be1 + c) : zero4();
    }
    if (live && q == 0 && meanc) {
      meanc[row] = mu;
      rstdc[row] = rs;
      mean1[row] = mu1;
      rstd1[row] = rs1;
    }
  }
  // (the first __syncthreads of the slice loop below orders these writes before the fragment reads)

  const int br = tid >> 2, bq4 = 4 * (tid & 3);  // Wq slice: output row tid / 4, four channels at 4 * (tid % 4)
  f4 vb;
  auto fetchq = [&](int o0, int c0) {
    const int o = o0 + br, c = c0 + bq4;
    vb = (o < O && c < C) ? ld4(wq + (int64_t)o * C + c) : zero4();
  };
  for (int o0 = 0; o0 < O; o0 += T) {
    f4 acc[2][2];
    clear_acc(acc);
    fetchq(o0, 0);
    for (int c0 = 0; c0 < Cr; c0 += KC) {
      *reinterpret_cast<f4*>(&Ws[br * kPitch + bq4]) = vb;
      __syncthreads();
      if (c0 + KC < Cr) fetchq(o0, c0 + KC);
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
        const int64_t row = row0 + g.wr + 16 * i + 4 * g.fk + v;
        if (row >= N) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const int o = o0 + g.wc + 16 * j + g.fl;
          if (o < O) qkv[row * qs + o] = acc[i][j][v] + bq[o];
        }
      }
  }
}

// ---- backward, the row tiles --------------------------------------------------------------------------------------------
// out[0][c] = sum_r d[r][c] h[r][c], out[1][c] = sum_r d[r][c] over the tile's live rows, d the LDS image and
// h = (src - mean) rstd read per row: thread (row group, f4 column) sums its RPG rows in order, then the groups in order.
// Gs holds the groups' partials; the caller keeps a __syncthreads between two calls.
template <int CT>
__device__ __forceinline__ void front_col_sums(const float* Ds, const float* __restrict__ src, int64_t ss, const float* sMean,
                                               const float* sRstd, int64_t row0, int64_t N, int C, float* Gs,
                                               float* __restrict__ out) {
  constexpr int XP = CT + 4, CQ = CT / 4, GROUPS = 256 / CQ, RPG = T / GROUPS;
  static_assert(GROUPS * 2 * CT <= T * kPitchG, "the column partials live in the chunk image");
  const int tid = threadIdx.x;
  {
    const int cq = tid % CQ, grp = tid / CQ, c = 4 * cq;
    f4 pg = zero4(), pb = zero4();
    if (c < C) {
#pragma unroll
      for (int k = 0; k < RPG; k++) {
        const int r = grp * RPG + k;
        if (row0 + r >= N) break;
        const f4 d = *reinterpret_cast<const f4*>(&Ds[r * XP + c]);
        const f4 h = (ld4(src + (row0 + r) * ss + c) - sMean[r]) * sRstd[r];
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
      out[which * C + c] = v;
    }
  }
}

// dt [N][C] is always written; dx, ds and lnpart [tiles][4][C] (column sums of dn o fhat, dn, df o that, df) when not null.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_front_bwd_rows(
    const float* __restrict__ feat, int64_t fs, const float* __restrict__ t, const float* __restrict__ meanc,
    const float* __restrict__ rstdc, const float* __restrict__ mean1, const float* __restrict__ rstd1,
    const float* __restrict__ dfeat, int64_t dfs, const float* __restrict__ dqkv, int64_t dqs, const float* __restrict__ wc,
    const float* __restrict__ gc, const float* __restrict__ g1, const float* __restrict__ wq, int64_t N, int C, int O,
    float* __restrict__ dx, int64_t dxs, float* __restrict__ ds, int64_t dss, float* __restrict__ dt, float* __restrict__ lnpart) {
  constexpr int CT = 32 * NJ, XP = CT + 4, WP = CT + 16, NV = NJ > 2 ? NJ / 2 : 1, CQ = CT / 4;
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];       // dn, then df, then dt: rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];  // dqkv of one chunk; then the column partials
  __shared__ __attribute__((aligned(16))) float Ws[KC * WP];      // a 16-deep slice of Wq, then of Wc: summed index in rows
  __shared__ float sM1[T], sR1[T], sMc[T], sRc[T];
  const int tid = threadIdx.x;
  const WaveTile g;
  const int wcn = (g.wc >> 5) * 16 * NJ;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC;

  if (tid < T) {
    const bool live = row0 + tid < N;
    sM1[tid] = live ? mean1[row0 + tid] : 0.0f;
    sR1[tid] = live ? rstd1[row0 + tid] : 0.0f;
    sMc[tid] = live ? meanc[row0 + tid] : 0.0f;
    sRc[tid] = live ? rstdc[row0 + tid] : 0.0f;
  }

  f4 vw[NV];
  auto fetchw = [&](const float* __restrict__ w, int rows, int k0) {  // slice of w [rows][C]: row k0 + e / CQ, four channels
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u, o = k0 + e / CQ, c = 4 * (e % CQ);
      vw[u] = (e < KC * CQ && o < rows && c < C) ? ld4(w + (int64_t)o * C + c) : zero4();
    }
  };
  auto put = [&]() {
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = tid + 256 * u;
      if (e < KC * CQ) *reinterpret_cast<f4*>(&Ws[(e / CQ) * WP + 4 * (e % CQ)]) = vw[u];
    }
  };

  f4 xacc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) xacc[i][j] = zero4();

  for (int o0 = 0; o0 < O; o0 += FH) {
    fetchw(wq, O, o0);
    // (the __syncthreads that closed the last chain is behind every read of the previous chunk's image)
    for (int e = tid; e < T * (FH / 4); e += 256) {
      const int r = e / (FH / 4), oc = 4 * (e % (FH / 4));
      *reinterpret_cast<f4*>(&Gs[r * kPitchG + oc]) =
          (row0 + r < N && o0 + oc < O) ? ld4(dqkv + (row0 + r) * dqs + o0 + oc) : zero4();
    }
    const int kend = O - o0 < FH ? (O - o0 + KC - 1) / KC * KC : FH;
    f4 tacc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < NJ; j++) tacc[i][j] = zero4();
    for (int k0 = 0; k0 < kend; k0 += KC) {
      put();
      __syncthreads();
      if (k0 + KC < kend) fetchw(wq, O, o0 + k0 + KC);
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

  // dn -> LDS (channels beyond C are zeros: their columns of Wq were staged as zeros)
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int rl = g.wr + 16 * i + 4 * g.fk + v;
#pragma unroll
      for (int j = 0; j < NJ; j++) Ds[rl * XP + wcn + 16 * j + g.fl] = xacc[i][j][v];
    }
  __syncthreads();

  float* lnrec = lnpart ? lnpart + (int64_t)blockIdx.x * 4 * C : nullptr;
  if (lnrec) front_col_sums<CT>(Ds, feat, fs, sM1, sR1, row0, N, C, Gs, lnrec);  // dg1, dbe1: before dn is overwritten

  const int r = tid >> 2, q = tid & 3;  // the LayerNorm backwards: lane q of a row owns the elements 4 q + 16 k .. + 3
  const int64_t row = row0 + r;
  const bool live = row < N;
  {  // LN_1: df = dfeat + rstd_1 (u - mean_c(u) - fhat mean_c(u fhat)), u = dn g1; a lane reads and writes its own elements
    const float mu = sM1[r], rs = sR1[r];
    f4 fh[2 * NJ], wd[2 * NJ];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      fh[k] = zero4();
      wd[k] = zero4();
      if (live && c < C) {
        fh[k] = (ld4(feat + row * fs + c) - mu) * rs;
        wd[k] = *reinterpret_cast<const f4*>(&Ds[r * XP + c]) * ld4(g1 + c);
        s1 = sum4(s1, wd[k]);
        s2 = sum4(s2, wd[k] * fh[k]);
      }
    }
    const float c1 = quad_sum(s1) / (float)C, c2 = quad_sum(s2) / (float)C;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      f4 df = zero4();
      if (live && c < C) {
        df = ld4(dfeat + row * dfs + c) + (wd[k] - c1 - fh[k] * c2) * rs;
        if (dx) st4(dx + row * dxs + c, df);
      }
      *reinterpret_cast<f4*>(&Ds[r * XP + c]) = df;
    }
  }
  __syncthreads();
  if (lnrec) front_col_sums<CT>(Ds, t, C, sMc, sRc, row0, N, C, Gs, lnrec + 2 * C);  // dgc, dbec
  {  // LN_c: dt = rstd_c (u - mean_c(u) - that mean_c(u that)), u = df gc
    const float mu = sMc[r], rs = sRc[r];
    f4 th[2 * NJ], wd[2 * NJ];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      th[k] = zero4();
      wd[k] = zero4();
      if (live && c < C) {
        th[k] = (ld4(t + row * C + c) - mu) * rs;
        wd[k] = *reinterpret_cast<const f4*>(&Ds[r * XP + c]) * ld4(gc + c);
        s1 = sum4(s1, wd[k]);
        s2 = sum4(s2, wd[k] * th[k]);
      }
    }
    const float c1 = quad_sum(s1) / (float)C, c2 = quad_sum(s2) / (float)C;
#pragma unroll
    for (int k = 0; k < 2 * NJ; k++) {
      const int c = 4 * q + 16 * k;
      f4 dv = zero4();
      if (live && c < C) {
        dv = (wd[k] - c1 - th[k] * c2) * rs;
        st4(dt + row * C + c, dv);
      }
      *reinterpret_cast<f4*>(&Ds[r * XP + c]) = dv;
    }
  }
  if (!ds) return;
  // (the first __syncthreads of the slice loop orders dt's image before the fragment reads)

  f4 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NJ; j++) acc[i][j] = zero4();
  fetchw(wc, C, 0);
  for (int k0 = 0; k0 < Cr; k0 += KC) {
    put();
    __syncthreads();
    if (k0 + KC < Cr) fetchw(wc, C, k0 + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      float fa[2], fb[NJ];
#pragma unroll
      for (int i = 0; i < 2; i++) fa[i] = Ds[(g.wr + 16 * i + g.fl) * XP + k0 + kk + g.fk];
#pragma unroll
      for (int j = 0; j < NJ; j++) fb[j] = Ws[(kk + g.fk) * WP + wcn + 16 * j + g.fl];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int64_t orow = row0 + g.wr + 16 * i + 4 * g.fk + v;
      if (orow >= N) continue;
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int c = wcn + 16 * j + g.fl;
        if (c < C) ds[orow * dss + c] = acc[i][j][v];
      }
    }
}

// ---- backward, the two weight gradients ---------------------------------------------------------------------------------
// A slice's record in `part`: dWq [O][C], dWc [C][C], dbq [O], dbc [C].
__host__ __device__ inline int64_t front_record(int C, int O) { return (int64_t)O * C + (int64_t)C * C + O + C; }

// MODE 0: dWq[o][c] = sum_r dqkv[r][o] n[r][c], dbq[o] = sum_r dqkv[r][o], n = (feat - mean_1) rstd_1 g1 + be1.
// MODE 1: dWc[o][c] = sum_r dt[r][o] s[r][c], dbc[o] = sum_r dt[r][o].  The sums are dw_slice_tile's (gcm_ffn.h).
template <int MODE>
__device__ __forceinline__ void front_dw_tile(const float* __restrict__ s, int64_t ss, const float* __restrict__ feat,
                                              int64_t fs, const float* __restrict__ mean1, const float* __restrict__ rstd1,
                                              const float* __restrict__ g1, const float* __restrict__ be1,
                                              const float* __restrict__ dqkv, int64_t dqs, const float* __restrict__ dt,
                                              int64_t N, int C, int O, int64_t per, float* __restrict__ rec, float* Ds,
                                              float* Xs) {
  const int Od = MODE == 0 ? O : C, I = C;
  const int tiles_i = (I + T - 1) / T;
  if ((int)blockIdx.x >= ((Od + T - 1) / T) * tiles_i) return;  // the grid is sized for the larger product
  const int o0 = (blockIdx.x / tiles_i) * T, i0 = (blockIdx.x % tiles_i) * T;
  const int64_t p0 = blockIdx.y * per, p1 = p0 + per < N ? p0 + per : N;
  const int sc = 4 * (threadIdx.x & 15);
  f4 gam = zero4(), bet = zero4();
  if (MODE == 0 && i0 + sc < I) {
    gam = ld4(g1 + i0 + sc);
    bet = ld4(be1 + i0 + sc);
  }
  auto fetch = [&](int64_t r, bool od, bool ix, f4& vd, f4& vx) {
    if (MODE == 0) {
      if (od) vd = ld4(dqkv + r * dqs + o0 + sc);
      if (ix) vx = (ld4(feat + r * fs + i0 + sc) - mean1[r]) * rstd1[r] * gam + bet;
    } else {
      if (od) vd = ld4(dt + r * C + o0 + sc);
      if (ix) vx = ld4(s + r * ss + i0 + sc);
    }
  };
  const int64_t OC = (int64_t)O * C, CC = (int64_t)C * C;
  dw_slice_tile(fetch, Od, I, o0, i0, p0, p1, rec + (MODE == 0 ? 0 : OC), rec + OC + CC + (MODE == 0 ? 0 : O), Ds, Xs);
}

// grid: (tiles of 64 x 64 over max(O, C) x C, row slices, the products asked for): mode z0 + z; 0 is dWq / dbq, 1 is dWc / dbc
__global__ __launch_bounds__(256) void k_front_dw(const float* __restrict__ s, int64_t ss, const float* __restrict__ feat,
                                                  int64_t fs, const float* __restrict__ mean1, const float* __restrict__ rstd1,
                                                  const float* __restrict__ g1, const float* __restrict__ be1,
                                                  const float* __restrict__ dqkv, int64_t dqs, const float* __restrict__ dt,
                                                  int64_t N, int C, int O, int64_t per, int z0, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ds[KC * kPitchT];
  __shared__ __attribute__((aligned(16))) float Xs[KC * kPitchT];
  float* rec = part + (int64_t)blockIdx.y * front_record(C, O);
  if (z0 + (int)blockIdx.z == 0) front_dw_tile<0>(s, ss, feat, fs, mean1, rstd1, g1, be1, dqkv, dqs, dt, N, C, O, per, rec, Ds, Xs);
  else front_dw_tile<1>(s, ss, feat, fs, mean1, rstd1, g1, be1, dqkv, dqs, dt, N, C, O, per, rec, Ds, Xs);
}

// dg1, dbe1, dgc, dbec: the records [4][C] in order
__global__ void k_front_fold_ln(const float* __restrict__ part, int64_t S, int C, float* __restrict__ dg1,
                                float* __restrict__ dbe1, float* __restrict__ dgc, float* __restrict__ dbec) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 4 * C) return;
  float* const outs[4] = {dg1, dbe1, dgc, dbec};
  float* out = outs[e / C];
  if (!out) return;
  float v = part[e];
  for (int64_t s = 1; s < S; s++) v += part[s * 4 * C + e];
  out[e % C] = v;
}

// ---- host: the plan and the launches ------------------------------------------------------------------------------------
struct FrontPlan {
  int64_t tiles;   // row tiles
  int64_t groups;  // first-level groups of the LayerNorm partials (0: one level)
  int64_t gper;    // tiles per group
  int sw;          // row slices of the weight gradients
  unsigned wt;     // 64 x 64 tiles of the larger weight gradient
  size_t dt, lnpart, lngroup, wpart, total;
};
FrontPlan front_plan(int64_t N, int32_t C, int32_t O) {
  FrontPlan p;
  p.tiles = (N + T - 1) / T;
  p.groups = p.tiles > kFfnFoldTiles ? std::min<int64_t>(256, (p.tiles + kFfnFoldTiles - 1) / kFfnFoldTiles) : 0;
  p.gper = p.groups ? (p.tiles + p.groups - 1) / p.groups : 0;
  p.wt = (unsigned)((std::max(O, C) + T - 1) / T) * (unsigned)((C + T - 1) / T);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kFfnMaxSlices, 1024 / p.wt));
  p.sw = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (N + 63) / 64));
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  p.dt = take((size_t)N * C * 4);
  p.lnpart = take((size_t)p.tiles * 4 * C * 4);
  p.lngroup = take((size_t)p.groups * 4 * C * 4);
  p.wpart = take((size_t)p.sw * (size_t)front_record(C, O) * 4);
  p.total = off;
  return p;
}

template <typename... A>
void front_launch_forward(int C, dim3 grid, hipStream_t st, A... args) {
  if (C <= 32) k_front_forward<1><<<grid, 256, 0, st>>>(args...);
  else if (C <= 64) k_front_forward<2><<<grid, 256, 0, st>>>(args...);
  else k_front_forward<4><<<grid, 256, 0, st>>>(args...);
}
template <typename... A>
void front_launch_bwd_rows(int C, dim3 grid, hipStream_t st, A... args) {
  if (C <= 32) k_front_bwd_rows<1><<<grid, 256, 0, st>>>(args...);
  else if (C <= 64) k_front_bwd_rows<2><<<grid, 256, 0, st>>>(args...);
  else k_front_bwd_rows<4><<<grid, 256, 0, st>>>(args...);
}

}  // namespace
