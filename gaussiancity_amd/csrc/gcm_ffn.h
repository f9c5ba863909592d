// gcm_ffn.h -- the feed-forward third of a PTv3 Block (gcm_ffn_* and gcm_ffn_split_*, include/gcm.h):
// y = x + s o (GELU(LN(x) W1^T + b1) W2^T + b2) and its deterministic backward in a handful of launches whatever N is.
// Included by gcm_modlinear.hip after gcm_tile.h, which holds the tile, the product loop and the LayerNorm lane rule; device
// code and the plan only, the C ABI stays in gcm_modlinear.hip.  DESIGN.md section 18.
//
// A workgroup owns T = 64 rows.  CT = 32 NJ NB is the channel width a kernel instantiation holds: NB column blocks of 32 NJ
// (NJ = 1, 2, 4 and NB = 1 up to 128 channels; NJ = 4 and NB = 2, 4 for CT = 256, 512).  C <= CT, channels beyond C and
// rows beyond N are staged as zeros, the summed index over the channels runs to C rounded up to 16 only.
//
// The arithmetic exists once, as __forceinline__ bodies (FfnRows .. ffn_ln_tail below) under two families of kernels:
//   forward   ffn_row_image: x tile -> LDS, normalised in place (4 lanes per row, fixed order).  ffn_forward_chunk, per
//             chunk of 64 hidden features: a = xn W1^T (one chain over C) + b1 -> stored when the caller asks ->
//             g = GELU(a) in registers -> LDS; per column block t_chunk = g W2^T (one chain from 0 over the chunk's 64
//             features), handed to the kernel's sink.  A wave's tile of a column block is 32 rows x 16 NJ channels.
//   backward  ffn_stage_dt: dt = s o dy -> LDS.  ffn_backward_chunk: dg = dt W2 (chain over C), da = dg o gelu'(a) ->
//             workspace and LDS, per column block dxn_chunk = da W1 (chain over the chunk) -> the sink.  ffn_ln_tail: from
//             dxn in LDS the LayerNorm backward per row, dx = dy + ..., and the tile's column sums of dxn o xhat and dxn
//             (row groups in ascending order).
//   one launch (gcm_ffn_*, C <= 128)  k_ffn_forward, k_ffn_bwd_rows: a workgroup walks every chunk, the sink adds the chunk
//             onto cleared accumulators in registers, and the kernel ends the operator itself: + b2, o s_r, + x; or dxn ->
//             LDS and the tail.
//   split (gcm_ffn_split_*, C <= 512)  the grid is (row tiles, hidden groups) and the second product leaves the workgroup as
//             a partial record [chunk][N][C] (SplitWalk); k_ffn_split_finish and k_ffn_split_bwd_ln add the records in
//             ascending chunk order from +0 -- the order the one-launch kernels add onto their cleared accumulators -- and
//             end the operator.  Two modes, chosen by the plan from N, C and Hd alone:
//               split  one chunk per workgroup, P = ceil(Hd / 64) records            (tiles x chunks <= kFfnSplitLimit)
//               rows   a workgroup walks all chunks and adds them in registers, P = 1 (the workspace stays bounded)
//             Every path is "per chunk one chain from 0, the chunks added in ascending order", so neither the mode nor the
//             family shows in the bits.  LDS is dynamic here: the row image alone is 132 096 bytes at CT = 512.
//   weights   k_ffn_dw: dW1 = da^T xn and dW2 = dt^T GELU(a) in row slices (k_modlinear_dw's scheme, both in one launch),
//             with db1 / db2 as the column sums of the slice's da / dt.  k_ffn_fold_params adds the slices pairwise, a fixed
//             tree; fold_ln_partials (gcm_tile.h) adds the tiles' LayerNorm partials in tile order.  Both families use them.
// Nothing depends on how many workgroups are resident: every sum has a fixed set of terms in a fixed order.
#pragma once
#include <atomic>

namespace {

constexpr int kFfnMaxChannels = 128;   // widest one-launch instantiation (NJ = 4)
constexpr int kFfnSumRows = 32;        // weight gradients: a chain runs over this many rows, the chains' results are added in order

// ---- the bodies both kernel families run -------------------------------------------------------------------------------
// The workgroup's row tile and the extents every body needs.  The bodies take it by value: behind a reference the widest
// rows-mode instantiations spent up to 90 more registers.
struct FfnRows {
  WaveTile g;
  int64_t row0, N;
  int C, Hd, Cr;  // Cr: C rounded up to whole slices, the extent of a chain over the channels
  __device__ __forceinline__ FfnRows(int64_t N_, int C_, int Hd_)
      : row0((int64_t)blockIdx.x * T), N(N_), C(C_), Hd(Hd_), Cr((C_ + KC - 1) / KC * KC) {}
};

// The row image: the tile's x rows -> Xs (pitch XP), LayerNorm in place.  Every workgroup of a tile forms the same
// statistics; the one whose `stores` holds writes mean and rstd, when they are not null.
__device__ __forceinline__ void ffn_row_image(const FfnRows t, float* Xs, int XP, const float* __restrict__ x, int64_t xs,
                                              const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                              bool stores, float* __restrict__ mean, float* __restrict__ rstd) {
  stage_rows(Xs, XP, t.Cr >> 2,
             [&](int r, int c) { return (t.row0 + r < t.N && c < t.C) ? ld4(x + (t.row0 + r) * xs + c) : zero4(); });
  __syncthreads();
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  const bool live = t.row0 + r < t.N;
  const RowStat st = ln_rows_forward(
      &Xs[r * XP], q, t.C, eps, [](int, f4) {}, [&](int c, f4 h) { return live ? h * ld4(lnw + c) + ld4(lnb + c) : zero4(); });
  if (live && q == 0 && mean && stores) {
    mean[t.row0 + r] = st.mean;
    rstd[t.row0 + r] = st.rstd;
  }
}

// The second product of a chunk, either direction.  Per column block nb with a live channel: tacc = Gs . wb_in(first column)
// as ONE chain from 0 over the chunk's features (whole slices of them: kend), then sink(nb, tacc) -- run() is never handed
// anything but a cleared tacc.  The caller has issued two.first(wb_in(0)) from the tail of the first product; the later
// blocks' first slices are fetched in front of their chains.
template <int NJ, int NB, bool TFORM, int WN, typename WB, typename Sink>
__device__ __forceinline__ void ffn_column_blocks(Chain<NJ, TFORM>& two, const FfnRows t, int h0, const float* Gs, float (&Ws)[WN],
                                                  WB wb_in, Sink sink) {
  constexpr int CB = 32 * NJ;
  const int kend = t.Hd - h0 < FH ? (t.Hd - h0 + KC - 1) / KC * KC : FH;
#pragma unroll
  for (int nb = 0; nb < NB; nb++) {
    if (NB == 1 || nb * CB < t.C) {  // else: a column block without a live channel
      f4 tacc[2][NJ];
      clear_acc(tacc);
      if (nb > 0) two.first(wb_in(nb * CB));
      two.run(tacc, t.g, Gs, kPitchG, kend, Ws, wb_in(nb * CB));
      sink(nb, tacc);
    }
  }
}

// One chunk of FH hidden features, forward: a = xn W1^T + b1 as one chain over the channels of the row image Xs (pitch
// 32 NJ NB + 4), stored when `a` is not null; g = GELU(a) -> Gs; then t = g W2^T per column block -> sink.
template <int NJ, int NB, int WN, typename Sink>
__device__ __forceinline__ void ffn_forward_chunk(const FfnRows t, int h0, const float* Xs, float* Gs, float (&Ws)[WN],
                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                  const float* __restrict__ w2, float* __restrict__ a, Sink sink) {
  const int64_t N = t.N;
  const int C = t.C, Hd = t.Hd;
  auto w1_at = [&](int hl, int c) { return (h0 + hl < Hd && c < C) ? ld4(w1 + (int64_t)(h0 + hl) * C + c) : zero4(); };
  auto w2_in = [&](int cb) {
    return [=](int c, int k) { return (cb + c < C && h0 + k < Hd) ? ld4(w2 + (int64_t)(cb + c) * Hd + h0 + k) : zero4(); };
  };
  Chain<2, false> up;     // the chunk's 64 hidden features, summed over the channels
  Chain<NJ, false> down;  // a column block, summed over the chunk's hidden features
  f4 acc[2][2];
  clear_acc(acc);
  up.first(w1_at);
  up.run(acc, t.g, Xs, 32 * NJ * NB + 4, t.Cr, Ws, w1_at, [&]() { down.first(w2_in(0)); });
  for_each_output(acc, t.g, [&](int rl, int hl, float v) {
    const int64_t row = t.row0 + rl;
    const int h = h0 + hl;
    float gv = 0.0f;
    if (h < Hd) {
      const float av = v + b1[h];
      if (a && row < N) a[row * Hd + h] = av;
      gv = gelu_f(av);
    }
    Gs[rl * kPitchG + hl] = gv;
  });
  ffn_column_blocks<NJ, NB>(down, t, h0, Gs, Ws, w2_in, sink);
}

// The same backward: dg = dt W2 as one chain over the channels of dt's image Ds, da = dg o gelu'(a) -> workspace (always)
// and Gs; then dxn = da W1 per column block -> sink.
template <int NJ, int NB, int WN, typename Sink>
__device__ __forceinline__ void ffn_backward_chunk(const FfnRows t, int h0, const float* Ds, float* Gs, float (&Ws)[WN],
                                                   const float* __restrict__ a, const float* __restrict__ w1,
                                                   const float* __restrict__ w2, float* __restrict__ da, Sink sink) {
  const int64_t N = t.N;
  const int C = t.C, Hd = t.Hd;
  auto w2_at = [&](int hl, int c) { return (c < C && h0 + hl < Hd) ? ld4(w2 + (int64_t)c * Hd + h0 + hl) : zero4(); };
  auto w1_in = [&](int cb) {
    return [=](int c, int k) { return (h0 + k < Hd && cb + c < C) ? ld4(w1 + (int64_t)(h0 + k) * C + cb + c) : zero4(); };
  };
  Chain<2, true> back2;   // the chunk's 64 hidden features, summed over the channels
  Chain<NJ, true> back1;  // a column block, summed over the chunk's hidden features
  f4 acc[2][2];
  clear_acc(acc);
  back2.first(w2_at);
  back2.run(acc, t.g, Ds, 32 * NJ * NB + 4, t.Cr, Ws, w2_at, [&]() { back1.first(w1_in(0)); });
  for_each_output(acc, t.g, [&](int rl, int hl, float v) {
    const int64_t row = t.row0 + rl;
    const int h = h0 + hl;
    float dv = 0.0f;
    if (h < Hd && row < N) {
      dv = v * gelu_grad_f(a[row * Hd + h]);
      da[row * Hd + h] = dv;
    }
    Gs[rl * kPitchG + hl] = dv;
  });
  ffn_column_blocks<NJ, NB>(back1, t, h0, Gs, Ws, w1_in, sink);
}

// the backward's row image dt = s o dy -> Ds (pitch XP), and the rows' saved statistics -> sMean, sRstd
__device__ __forceinline__ void ffn_stage_dt(const FfnRows t, float* Ds, int XP, const float* __restrict__ dy, int64_t dys,
                                             const float* __restrict__ s) {
  stage_rows(Ds, XP, t.Cr >> 2, [&](int r, int c) {
    f4 v = zero4();
    if (t.row0 + r < t.N && c < t.C) {
      v = ld4(dy + (t.row0 + r) * dys + c);
      if (s) v = v * s[t.row0 + r];
    }
    return v;
  });
}
__device__ __forceinline__ void ffn_load_stats(const FfnRows t, const float* __restrict__ mean, const float* __restrict__ rstd,
                                               float* sMean, float* sRstd) {
  const int tid = threadIdx.x;
  if (tid < T) {
    const bool live = t.row0 + tid < t.N;
    sMean[tid] = live ? mean[t.row0 + tid] : 0.0f;
    sRstd[tid] = live ? rstd[t.row0 + tid] : 0.0f;
  }
}

// The end of the backward's row side, from dxn in Ds (pitch 32 NJ NB + 4; written by the caller, the barrier is here) and
// the statistics in sMean / sRstd: the LayerNorm backward per row and dx = dy + ... when dx is not null (in registers up to
// 128 channels, re-reading beyond), the tile's column sums into lnpart [tiles][2][C] when that is not null.
template <int NJ, int NB>
__device__ __forceinline__ void ffn_ln_tail(const FfnRows t, const float* Ds, float* Gs, const float* sMean, const float* sRstd,
                                            const float* __restrict__ x, int64_t xs, const float* __restrict__ dy, int64_t dys,
                                            const float* __restrict__ lnw, float* __restrict__ dx, int64_t dxs,
                                            float* __restrict__ lnpart) {
  constexpr int CT = 32 * NJ * NB, XP = CT + 4;
  __syncthreads();
  if (dx) {
    const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
    const int64_t row = t.row0 + r;
    auto src = [&](int c) { return ld4(x + row * xs + c); };
    auto out = [&](int c, f4 v) { st4(dx + row * dxs + c, ld4(dy + row * dys + c) + v); };
    if constexpr (NB == 1) ln_rows_backward<NJ>(&Ds[r * XP], q, t.C, row < t.N, {sMean[r], sRstd[r]}, lnw, src, out, [](int) {});
    else ln_rows_backward_reread(&Ds[r * XP], q, t.C, row < t.N, {sMean[r], sRstd[r]}, lnw, src, out);
  }
  if (lnpart) ln_col_sums<CT>(Ds, x, xs, sMean, sRstd, t.row0, t.N, t.C, Gs, lnpart + (int64_t)blockIdx.x * 2 * t.C);
}

// ---- one launch per direction, up to 128 channels -------------------------------------------------------------------------
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_ffn_forward(const float* __restrict__ x, int64_t xs, const float* __restrict__ lnw,
                                                        const float* __restrict__ lnb, float eps, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, const float* __restrict__ s, int64_t N,
                                                        int C, int Hd, float* __restrict__ y, int64_t ys,
                                                        float* __restrict__ mean, float* __restrict__ rstd,
                                                        float* __restrict__ a) {
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];                    // x, then LN(x): rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];               // GELU(a) of one chunk: rows x hidden
  __shared__ __attribute__((aligned(16))) float Ws[(CT > T ? CT : T) * kPitch];  // a 16-deep slice of W1, then of W2
  const FfnRows t(N, C, Hd);
  ffn_row_image(t, Xs, XP, x, xs, lnw, lnb, eps, true, mean, rstd);

  f4 yacc[2][NJ];
  clear_acc(yacc);
  for (int h0 = 0; h0 < Hd; h0 += FH)
    ffn_forward_chunk<NJ, 1>(t, h0, Xs, Gs, Ws, w1, b1, w2, a, [&](int, const f4(&tacc)[2][NJ]) { add_acc(yacc, tacc); });

  for_each_output(
      yacc, t.g, [&](int rl) { return scaled_row(t.row0 + rl, N, s); },
      [&](ScaledRow r, int c, float v) {
        if (r.row < 0 || c >= C) return;
        const float tv = v + b2[c];
        y[r.row * ys + c] = x[r.row * xs + c] + (s ? r.scale * tv : tv);
      });
}

// da [N][Hd] is always written; dx and lnpart [tiles][2][C] (column sums of dxn o xhat, then of dxn) when not null.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_ffn_bwd_rows(const float* __restrict__ x, int64_t xs, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ a,
                                                         const float* __restrict__ dy, int64_t dys, const float* __restrict__ s,
                                                         const float* __restrict__ lnw, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, int64_t N, int C, int Hd,
                                                         float* __restrict__ dx, int64_t dxs, float* __restrict__ da,
                                                         float* __restrict__ lnpart) {
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];                    // dt, then dxn: rows x channels
  __shared__ __attribute__((aligned(16))) float Gs[T * kPitchG];               // da of one chunk; then the column partials
  __shared__ __attribute__((aligned(16))) float Ws[KC * ((CT > T ? CT : T) + 16)];  // a slice of W2, then of W1
  __shared__ float sMean[T], sRstd[T];
  const FfnRows t(N, C, Hd);
  ffn_load_stats(t, mean, rstd, sMean, sRstd);
  ffn_stage_dt(t, Ds, XP, dy, dys, s);

  f4 xacc[2][NJ];
  clear_acc(xacc);
  for (int h0 = 0; h0 < Hd; h0 += FH)
    ffn_backward_chunk<NJ, 1>(t, h0, Ds, Gs, Ws, a, w1, w2, da, [&](int, const f4(&tacc)[2][NJ]) { add_acc(xacc, tacc); });

  for_each_output(xacc, t.g, [&](int rl, int c, float v) { Ds[rl * XP + c] = v; });  // dxn over dt's image
  ffn_ln_tail<NJ, 1>(t, Ds, Gs, sMean, sRstd, x, xs, dy, dys, lnw, dx, dxs, lnpart);
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
    add_acc(tot, acc);
    clear_acc(acc);
    btot += bsum;
    bsum = 0.0f;
  };
  fetch(p0);
  for (int64_t p = p0; p < p1; p += KC) {
    if (p != p0 && (p - p0) % kFfnSumRows == 0) flush();
    st4(&Ds[sp * kPitchT + sc], vd);
    st4(&Xs[sp * kPitchT + sc], vx);
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
  for_each_output(tot, g, [&](int ol, int cl, float v) {
    if (o0 + ol < Od && i0 + cl < I) dst[(int64_t)(o0 + ol) * I + i0 + cl] = v;
  });
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

// ---- up to 512 channels, the hidden width split across workgroups (gcm_ffn_split_*) ---------------------------------------
#ifndef GCM_FFN_SPLIT_LIMIT
#define GCM_FFN_SPLIT_LIMIT 2048
#endif
constexpr int kFfnSplitMaxChannels = 512;
constexpr int64_t kFfnSplitLimit = GCM_FFN_SPLIT_LIMIT;  // tiles x chunks beyond which a workgroup walks its chunks

constexpr int split_slice_cols(int NJ) { return 32 * NJ > T ? 32 * NJ : T; }
constexpr size_t split_fwd_lds(int NJ, int NB) { return (size_t)(T * (32 * NJ * NB + 4) + T * kPitchG + split_slice_cols(NJ) * kPitch) * 4; }
constexpr size_t split_bwd_lds(int NJ, int NB) { return (size_t)(T * (32 * NJ * NB + 4) + T * kPitchG + KC * (split_slice_cols(NJ) + 16)) * 4; }
constexpr size_t split_ln_lds(int NJ, int NB) { return (size_t)(T * (32 * NJ * NB + 4) + T * kPitchG) * 4; }

// part[rec][row][c] = acc for the tile's live rows and the live columns of column block cb
template <int NJ>
__device__ __forceinline__ void split_store(const f4 (&acc)[2][NJ], const WaveTile& g, float* __restrict__ part, int64_t rec,
                                            int64_t row0, int64_t N, int C, int cb) {
  for_each_output(acc, g, [&](int rl, int cl, float v) {
    const int64_t row = row0 + rl;
    const int c = cb + cl;
    if (row < N && c < C) part[(rec * N + row) * C + c] = v;
  });
}

// the P records' four floats at `at` (a record is `rs` floats) added in ascending order from +0; the loads of up to 16
// records are in flight together, the adds are one chain
__device__ __forceinline__ f4 split_fold(const float* __restrict__ at, int64_t rs, int P) {
  f4 v = zero4();
  int p = 0;
  for (; p + 16 <= P; p += 16) {
    f4 t[16];
#pragma unroll
    for (int k = 0; k < 16; k++) t[k] = ld4(at + (p + k) * rs);
#pragma unroll
    for (int k = 0; k < 16; k++) v = v + t[k];
  }
  for (; p + 4 <= P; p += 4) {
    f4 t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) t[k] = ld4(at + (p + k) * rs);
#pragma unroll
    for (int k = 0; k < 4; k++) v = v + t[k];
  }
  for (; p < P; p++) v = v + ld4(at + p * rs);
  return v;
}

// Which chunks a workgroup of the grid (row tiles, SPLIT ? chunks : 1) walks, hbeg .. hend, and where their second products
// go.  SPLIT: the chunk blockIdx.y, each column block into the chunk's record.  Rows mode: every chunk, added in ascending
// order onto cleared accumulators, which finish() puts into record 0.
template <int NJ, int NB, bool SPLIT>
struct SplitWalk {
  static constexpr int CB = 32 * NJ;
  const FfnRows& t;
  float* __restrict__ part;
  int hbeg, hend;
  f4 sum[SPLIT ? 1 : NB][2][NJ];
  __device__ __forceinline__ SplitWalk(const FfnRows& t_, float* part_) : t(t_), part(part_) {
    hbeg = SPLIT ? (int)blockIdx.y * FH : 0;
    hend = SPLIT ? (hbeg + FH < t.Hd ? hbeg + FH : t.Hd) : t.Hd;
    if (!SPLIT)
#pragma unroll
      for (int nb = 0; nb < NB; nb++) clear_acc(sum[nb]);
  }
  // Where chunk h0's column blocks go.  SPLIT: the callable holds copies of what it needs and nothing of this object --
  // read through the object, N and C were loaded again after every store to `part` and each record address was formed
  // anew: a fifth more instructions at CT = 512 and 3 % of the forward's time.
  __device__ __forceinline__ auto sink(int h0) {
    if constexpr (SPLIT) {
      const FfnRows r = t;
      float* p = part;
      return [=](int nb, const f4(&tacc)[2][NJ]) { split_store(tacc, r.g, p, h0 / FH, r.row0, r.N, r.C, nb * CB); };
    } else {
      return [this](int nb, const f4(&tacc)[2][NJ]) { add_acc(sum[nb], tacc); };
    }
  }
  __device__ __forceinline__ void finish() {
    if (!SPLIT)
#pragma unroll
      for (int nb = 0; nb < NB; nb++) split_store(sum[nb], t.g, part, 0, t.row0, t.N, t.C, nb * CB);
  }
};

// the chunks' t as partial records; mean, rstd (from the workgroups of group 0) and a when not null
template <int NJ, int NB, bool SPLIT>
__global__ __launch_bounds__(256, NB > 1 ? 1 : 2) void k_ffn_split_forward(
    const float* __restrict__ x, int64_t xs, const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, int64_t N, int C, int Hd,
    float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ a, float* __restrict__ part) {
  constexpr int XP = 32 * NJ * NB + 4, WN = split_slice_cols(NJ) * kPitch;
  extern __shared__ __attribute__((aligned(16))) float split_lds[];
  float* Xs = split_lds;                                                // x, then LN(x): rows x channels
  float* Gs = Xs + T * XP;                                              // GELU(a) of one chunk: rows x hidden
  float(&Ws)[WN] = *reinterpret_cast<float(*)[WN]>(Gs + T * kPitchG);   // a 16-deep slice of W1, then of W2
  const FfnRows t(N, C, Hd);
  ffn_row_image(t, Xs, XP, x, xs, lnw, lnb, eps, blockIdx.y == 0, mean, rstd);
  SplitWalk<NJ, NB, SPLIT> walk(t, part);
  for (int h0 = walk.hbeg; h0 < walk.hend; h0 += FH)
    ffn_forward_chunk<NJ, NB>(t, h0, Xs, Gs, Ws, w1, b1, w2, a, walk.sink(h0));
  walk.finish();
}

// y = x + s_r ((the P records added in ascending order from +0) + b2): one thread per four channels of a row
__global__ void k_ffn_split_finish(const float* __restrict__ part, int P, const float* __restrict__ x, int64_t xs,
                                   const float* __restrict__ b2, const float* __restrict__ s, int64_t N, int C,
                                   float* __restrict__ y, int64_t ys) {
  const int c4 = C >> 2;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * c4) return;
  const int64_t row = e / c4;
  const int c = 4 * (int)(e % c4);
  const f4 t = split_fold(part + row * C + c, N * C, P) + ld4(b2 + c);
  st4(y + row * ys + c, ld4(x + row * xs + c) + (s ? t * s[row] : t));
}

// da [N][Hd] for the workgroup's chunk(s), and the chunks' dxn as partial records
template <int NJ, int NB, bool SPLIT>
__global__ __launch_bounds__(256, NB > 1 ? 1 : 2) void k_ffn_split_bwd_rows(
    const float* __restrict__ a, const float* __restrict__ dy, int64_t dys, const float* __restrict__ s,
    const float* __restrict__ w1, const float* __restrict__ w2, int64_t N, int C, int Hd, float* __restrict__ da,
    float* __restrict__ part) {
  constexpr int XP = 32 * NJ * NB + 4, WN = KC * (split_slice_cols(NJ) + 16);
  extern __shared__ __attribute__((aligned(16))) float split_lds[];
  float* Ds = split_lds;                                                // dt: rows x channels
  float* Gs = Ds + T * XP;                                              // da of one chunk
  float(&Ws)[WN] = *reinterpret_cast<float(*)[WN]>(Gs + T * kPitchG);   // a slice of W2, then of W1
  const FfnRows t(N, C, Hd);
  ffn_stage_dt(t, Ds, XP, dy, dys, s);
  SplitWalk<NJ, NB, SPLIT> walk(t, part);
  for (int h0 = walk.hbeg; h0 < walk.hend; h0 += FH)
    ffn_backward_chunk<NJ, NB>(t, h0, Ds, Gs, Ws, a, w1, w2, da, walk.sink(h0));
  walk.finish();
}

// per row tile: dxn = the P records added in ascending order from +0 -> LDS, then the tail k_ffn_bwd_rows ends with
template <int NJ, int NB>
__global__ __launch_bounds__(256, NB > 1 ? 1 : 2) void k_ffn_split_bwd_ln(
    const float* __restrict__ part, int P, const float* __restrict__ x, int64_t xs, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ dy, int64_t dys, const float* __restrict__ lnw, int64_t N, int C,
    float* __restrict__ dx, int64_t dxs, float* __restrict__ lnpart) {
  constexpr int XP = 32 * NJ * NB + 4;
  extern __shared__ __attribute__((aligned(16))) float split_lds[];
  float* Ds = split_lds;       // dxn: rows x channels
  float* Gs = Ds + T * XP;     // the column partials
  __shared__ float sMean[T], sRstd[T];
  const FfnRows t(N, C, 0);  // no hidden width is walked here
  ffn_load_stats(t, mean, rstd, sMean, sRstd);
  stage_rows(Ds, XP, t.Cr >> 2, [&](int r, int c) {
    return (t.row0 + r < N && c < C) ? split_fold(part + (t.row0 + r) * C + c, N * C, P) : zero4();
  });
  ffn_ln_tail<NJ, NB>(t, Ds, Gs, sMean, sRstd, x, xs, dy, dys, lnw, dx, dxs, lnpart);
}

// ---- host: the plan and the launches ------------------------------------------------------------------------------------
// f(std::integral_constant<int, NJ>, std::integral_constant<int, NB>) for the narrowest instantiation that holds C
template <typename F>
void with_split_width(int C, F f) {
  if (C <= 128) with_nj(C, [&](auto nj) { f(nj, std::integral_constant<int, 1>{}); });
  else if (C <= 256) f(std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
}

// One plan for both families.  with_records: the split entry points, whose row-side kernels leave P partial records; the
// one-launch entry points are the case "no records, no forward workspace" (records = 0, `part` an empty piece).
struct FfnPlan {
  bool split;      // one chunk per workgroup
  int64_t tiles, chunks, records;  // row tiles, chunks of 64 hidden features, partial records P
  int64_t groups;  // first-level groups of the LayerNorm partials (0: one level)
  int64_t gper;    // tiles per group
  int sw;          // row slices of the weight gradients
  size_t fwd_total;                // the forward's workspace: the records of t
  size_t da, part, lnpart, lngroup, wpart, total;  // the backward's carve
};
FfnPlan ffn_plan(int64_t N, int32_t C, int32_t Hd, bool with_records) {
  FfnPlan p;
  p.tiles = (N + T - 1) / T;
  p.chunks = (Hd + FH - 1) / FH;
  p.split = with_records && p.tiles * p.chunks <= kFfnSplitLimit;
  p.records = !with_records ? 0 : p.split ? p.chunks : 1;
  fold_groups(p.tiles, p.groups, p.gper);
  p.sw = weight_slices((int64_t)((Hd + T - 1) / T) * ((C + T - 1) / T), N);
  const size_t rec = (size_t)p.records * (size_t)N * C * 4;
  p.fwd_total = round256(rec);
  Carve ws;
  p.da = ws.take((size_t)N * Hd * 4);
  p.part = ws.take(rec);
  p.lnpart = ws.take((size_t)p.tiles * 2 * C * 4);
  p.lngroup = ws.take((size_t)p.groups * 2 * C * 4);
  p.wpart = ws.take((size_t)p.sw * (size_t)ffn_record(C, Hd) * 4);
  p.total = ws.off;
  return p;
}

// more than 64 KB of dynamic LDS has to be asked for, per kernel and per device (asking twice is harmless): the
// instantiations of CT = 256 and 512
hipError_t split_lds_attr() {
  constexpr int kDevices = 64;
  static std::atomic<bool> done[kDevices];
  int dev = 0;
  if (const hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  const bool known = dev >= 0 && dev < kDevices;
  if (known && done[dev].load(std::memory_order_acquire)) return hipSuccess;
  hipError_t err = hipSuccess;
  auto ask = [&](const void* f, size_t bytes) {
    if (err == hipSuccess) err = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  };
  auto wide = [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    ask((const void*)k_ffn_split_forward<4, NB, true>, split_fwd_lds(4, NB));
    ask((const void*)k_ffn_split_forward<4, NB, false>, split_fwd_lds(4, NB));
    ask((const void*)k_ffn_split_bwd_rows<4, NB, true>, split_bwd_lds(4, NB));
    ask((const void*)k_ffn_split_bwd_rows<4, NB, false>, split_bwd_lds(4, NB));
    ask((const void*)k_ffn_split_bwd_ln<4, NB>, split_ln_lds(4, NB));
  };
  wide(std::integral_constant<int, 2>{});
  wide(std::integral_constant<int, 4>{});
  if (err == hipSuccess && known) done[dev].store(true, std::memory_order_release);
  return err;
}

}  // namespace
