// gcm_front.h -- the front of a PTv3 Block between its sparse convolution and its attention (gcm_front_*, include/gcm.h):
// t = s Wc^T + bc, feat = x + LN_c(t), qkv = LN_1(feat) Wq^T + bq in ONE launch, and its deterministic backward in four
// launches (five beyond 64 row tiles) whatever N is.  Included by gcm_modlinear.hip after gcm_tile.h (the tile, the product
// loop, the LayerNorm lane rule) and gcm_ffn.h (the row-sliced weight gradients); device code and the plan only, the C ABI
// stays in gcm_modlinear.hip.  DESIGN.md section 19.
//
// A workgroup owns T = 64 rows; CT = 32 NJ (NJ = 1, 2, 4) is the channel width an instantiation holds, C <= CT, channels
// beyond C and rows beyond N are zeros, the summed index over the channels runs to C rounded up to 16 only.
//   forward   s tile -> LDS; t accumulators (a wave's 32 rows x 16 NJ channels, one chain over C) stay in registers until
//             every wave has read s, then t + bc overwrites the tile.  Four lanes per row: LN_c, feat = x + u stored and
//             written back to the tile, LN_1 in place.  qkv per chunk of 64 outputs: one chain over C, + bq, stored.
//   backward  k_front_bwd_rows: per chunk of 64 outputs dqkv -> LDS, dn accumulators += dqkv_chunk Wq (one chain over the
//             chunk); dn -> LDS; the tile's column sums of dn o fhat and dn; LN_1 backward per row with feat read per row,
//             df = dfeat + ..., stored as dx and written back; the column sums of df o that and df; LN_c backward per row
//             with t read per row, dt -> workspace and LDS; ds = dt Wc (one chain over C) from the LDS image.
//             k_front_dw: dWq = dqkv^T n (n rebuilt from feat and LN_1's statistics) and dWc = dt^T s in row slices, both
//             in one launch, with dbq / dbc as the column sums of the slice's dqkv / dt.  k_ffn_fold_params adds the
//             slices pairwise, a fixed tree; fold_ln_partials adds the tiles' partials of BOTH LayerNorms (a record is
//             [4][C]: dg1, dbe1, dgc, dbec) in tile order, one launch per level.
// Nothing depends on how many workgroups are resident: every sum has a fixed set of terms in a fixed order.
#pragma once

namespace {

constexpr int kFrontMaxChannels = kFfnMaxChannels;  // widest instantiation (NJ = 4); O up to three times that

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
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];                      // s, then t, feat and LN_1(feat): rows x channels
  __shared__ __attribute__((aligned(16))) float Ws[(CT > T ? CT : T) * kPitch];  // a 16-deep slice of Wc, then of Wq
  const int tid = threadIdx.x;
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC;

  stage_rows(Xs, XP, Cr >> 2, [&](int r, int c) { return (row0 + r < N && c < C) ? ld4(s + (row0 + r) * ss + c) : zero4(); });

  {
    Chain<NJ, false> conv;  // t = s Wc^T
    auto wc_at = [&](int c, int k) { return (c < C && k < C) ? ld4(wc + (int64_t)c * C + k) : zero4(); };
    f4 tacc[2][NJ];
    clear_acc(tacc);
    conv.first(wc_at);
    conv.run(tacc, g, Xs, XP, Cr, Ws, wc_at);
    // every wave is past its last read of s: t + bc over the tile (channels beyond C stay zeros for the chain of qkv)
    for_each_output(tacc, g, [&](int rl, int c, float v) { Xs[rl * XP + c] = c < C ? v + bc[c] : 0.0f; });
  }
  __syncthreads();

  {  // the two LayerNorms in place
    const int r = tid >> 2, q = tid & 3;
    const int64_t row = row0 + r;
    const bool live = row < N;
    const RowStat sc = ln_rows_forward(
        &Xs[r * XP], q, C, epsc,
        [&](int c, f4 v) {
          if (t && live) st4(t + row * C + c, v);
        },
        [&](int c, f4 h) {
          f4 f = zero4();
          if (live) {
            f = ld4(x + row * xs + c) + (h * ld4(gc + c) + ld4(bec + c));
            st4(feat + row * fs + c, f);
          }
          return f;
        });
    const RowStat s1 = ln_rows_forward(
        &Xs[r * XP], q, C, eps1, [](int, f4) {}, [&](int c, f4 h) { return live ? h * ld4(g1 + c) + ld4(be1 + c) : zero4(); });
    if (live && q == 0 && meanc) {
      meanc[row] = sc.mean;
      rstdc[row] = sc.rstd;
      mean1[row] = s1.mean;
      rstd1[row] = s1.rstd;
    }
  }

  Chain<2, false> proj;  // qkv = n Wq^T, 64 outputs a chunk
  for (int o0 = 0; o0 < O; o0 += T) {
    auto wq_at = [&](int ol, int c) { return (o0 + ol < O && c < C) ? ld4(wq + (int64_t)(o0 + ol) * C + c) : zero4(); };
    f4 acc[2][2];
    clear_acc(acc);
    proj.first(wq_at);
    proj.run(acc, g, Xs, XP, Cr, Ws, wq_at);
    for_each_output(acc, g, [&](int rl, int ol, float v) {
      const int64_t row = row0 + rl;
      const int o = o0 + ol;
      if (row < N && o < O) qkv[row * qs + o] = v + bq[o];
    });
  }
}

// ---- backward, the row tiles --------------------------------------------------------------------------------------------
// dt [N][C] is always written; dx, ds and lnpart [tiles][4][C] (column sums of dn o fhat, dn, df o that, df) when not null.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_front_bwd_rows(
    const float* __restrict__ feat, int64_t fs, const float* __restrict__ t, const float* __restrict__ meanc,
    const float* __restrict__ rstdc, const float* __restrict__ mean1, const float* __restrict__ rstd1,
    const float* __restrict__ dfeat, int64_t dfs, const float* __restrict__ dqkv, int64_t dqs, const float* __restrict__ wc,
    const float* __restrict__ gc, const float* __restrict__ g1, const float* __restrict__ wq, int64_t N, int C, int O,
    float* __restrict__ dx, int64_t dxs, float* __restrict__ ds, int64_t dss, float* __restrict__ dt, float* __restrict__ lnpart) {
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];       // dn, then df, then dt: rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];  // dqkv of one chunk; then the column partials
  __shared__ __attribute__((aligned(16))) float Ws[Chain<NJ, true>::kWords];  // a 16-deep slice of Wq, then of Wc
  __shared__ float sM1[T], sR1[T], sMc[T], sRc[T];
  const int tid = threadIdx.x;
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC;

  if (tid < T) {
    const bool live = row0 + tid < N;
    sM1[tid] = live ? mean1[row0 + tid] : 0.0f;
    sR1[tid] = live ? rstd1[row0 + tid] : 0.0f;
    sMc[tid] = live ? meanc[row0 + tid] : 0.0f;
    sRc[tid] = live ? rstdc[row0 + tid] : 0.0f;
  }

  Chain<NJ, true> back;  // dn = dqkv Wq per chunk, then ds = dt Wc
  f4 xacc[2][NJ];
  clear_acc(xacc);
  for (int o0 = 0; o0 < O; o0 += FH) {
    auto wq_at = [&](int c, int k) { return (o0 + k < O && c < C) ? ld4(wq + (int64_t)(o0 + k) * C + c) : zero4(); };
    back.first(wq_at);
    // (the __syncthreads that closed the last chain is behind every read of the previous chunk's image)
    stage_rows(Gs, kPitchG, FH / 4, [&](int r, int oc) {
      return (row0 + r < N && o0 + oc < O) ? ld4(dqkv + (row0 + r) * dqs + o0 + oc) : zero4();
    });
    const int kend = O - o0 < FH ? (O - o0 + KC - 1) / KC * KC : FH;
    f4 tacc[2][NJ];
    clear_acc(tacc);
    back.run(tacc, g, Gs, kPitchG, kend, Ws, wq_at);
    add_acc(xacc, tacc);
  }

  // dn -> LDS (channels beyond C are zeros: their columns of Wq were staged as zeros)
  for_each_output(xacc, g, [&](int rl, int c, float v) { Ds[rl * XP + c] = v; });
  __syncthreads();

  float* lnrec = lnpart ? lnpart + (int64_t)blockIdx.x * 4 * C : nullptr;
  if (lnrec) ln_col_sums<CT>(Ds, feat, fs, sM1, sR1, row0, N, C, Gs, lnrec);  // dg1, dbe1: before dn is overwritten

  const int r = tid >> 2, q = tid & 3;
  const int64_t row = row0 + r;
  const bool live = row < N;
  // LN_1: df = dfeat + rstd_1 (u - mean_c(u) - fhat mean_c(u fhat)), u = dn g1; a lane reads and writes its own elements
  ln_rows_backward<NJ>(
      &Ds[r * XP], q, C, live, {sM1[r], sR1[r]}, g1, [&](int c) { return ld4(feat + row * fs + c); },
      [&](int c, f4 v) {
        const f4 df = ld4(dfeat + row * dfs + c) + v;
        if (dx) st4(dx + row * dxs + c, df);
        st4(&Ds[r * XP + c], df);
      },
      [&](int c) { st4(&Ds[r * XP + c], zero4()); });
  __syncthreads();
  if (lnrec) ln_col_sums<CT>(Ds, t, C, sMc, sRc, row0, N, C, Gs, lnrec + 2 * C);  // dgc, dbec
  // LN_c: dt = rstd_c (u - mean_c(u) - that mean_c(u that)), u = df gc
  ln_rows_backward<NJ>(
      &Ds[r * XP], q, C, live, {sMc[r], sRc[r]}, gc, [&](int c) { return ld4(t + row * C + c); },
      [&](int c, f4 v) {
        st4(dt + row * C + c, v);
        st4(&Ds[r * XP + c], v);
      },
      [&](int c) { st4(&Ds[r * XP + c], zero4()); });
  if (!ds) return;

  auto wc_at = [&](int c, int k) { return (k < C && c < C) ? ld4(wc + (int64_t)k * C + c) : zero4(); };
  f4 acc[2][NJ];
  clear_acc(acc);
  back.first(wc_at);
  back.run(acc, g, Ds, XP, Cr, Ws, wc_at);
  for_each_output(acc, g, [&](int rl, int c, float v) {
    const int64_t orow = row0 + rl;
    if (orow < N && c < C) ds[orow * dss + c] = v;
  });
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

// ---- host: the plan -------------------------------------------------------------------------------------------------------
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
  fold_groups(p.tiles, p.groups, p.gper);
  p.wt = (unsigned)((std::max(O, C) + T - 1) / T) * (unsigned)((C + T - 1) / T);
  p.sw = weight_slices(p.wt, N);
  Carve ws;
  p.dt = ws.take((size_t)N * C * 4);
  p.lnpart = ws.take((size_t)p.tiles * 4 * C * 4);
  p.lngroup = ws.take((size_t)p.groups * 4 * C * 4);
  p.wpart = ws.take((size_t)p.sw * (size_t)front_record(C, O) * 4);
  p.total = ws.off;
  return p;
}

}  // namespace
