// gcm_seam.h -- the seams between the PTv3 stages (gcm_seam_*, include/gcm.h): Linear -> BatchNorm1d -> GELU as one
// operator, y = act(bn(x W^T + b)), up to 512 channels either way; eval mode in ONE launch, training mode in three, the
// deterministic backward in five, whatever N is.  Included by gcm_modlinear.hip after gcm_tile.h (the tile and the
// product loop) and gcm_ffn.h (the row-sliced weight gradient); device code and the plans only, the C ABI stays in
// gcm_modlinear.hip.
// DESIGN.md section 21.
//
//   product    k_seam_forward: 256 threads own T = 64 rows and a block of CT = 32 NJ <= 128 output columns (grid.y walks
//              the blocks); the inputs are walked in chunks of <= 128 staged in LDS, the accumulators carry across the
//              chunks: z is one fp32 chain from 0 over the inputs in ascending order, b added after the chain.  The tile
//              of z goes through LDS: from there it is stored in 16-byte pieces (training) or normalised and stored as y
//              (eval), and a thread per column walks the tile's valid rows in ascending order: the mean (taken about the
//              tile's first row), then, about that mean, the centred second moment M2.  A tile's record in the workspace:
//              [2][O] = mean, M2 (the count of tile t is min(64, N - 64 t)).
//   statistics k_seam_stats: per column two passes over the tiles' records in ascending tile order: the mean, a compensated
//              sum of count_t mean_t divided by N, then M2 = sum_t (M2_t + count_t (mean_t - mean)^2), compensated (never
//              sum z^2 - (sum z)^2 / N); beyond 64 tiles, G <= 64 groups of consecutive tiles are summed first (each by
//              one thread, the same launch) and the groups then in ascending order.
//   apply      k_seam_apply: y = act(((z - mean) rstd) g + h), 16-byte accesses.
//   backward   k_seam_bwd_part / k_seam_bwd_fold: dh = sum du, dg = sum du zhat, per tile four chains of 16 rows added in
//              order, the tiles in ascending order with a compensated sum (grouped as the statistics).  k_seam_dx: dz
//              recomputed into LDS per 64 rows and chunk of <= 128 outputs, never stored; dx is, PER CHUNK, one fp32 chain
//              from 0 over the chunk's outputs in ascending order, the chunks' results added in ascending order.
//              k_seam_dw: dw_slice_tile with a fetch that recomputes dz, then k_ffn_fold_params' pairwise tree.
// Channels beyond I / O and rows beyond N are staged as zeros and never stored.
#pragma once

namespace {

constexpr int kSeamMaxChannels = 512;
constexpr int kSeamChunk = 128;      // inputs (forward) or outputs (dx) staged at a time
constexpr int kSeamFoldTiles = 64;   // up to this many tiles fold in one level
constexpr int kSeamGroups = 64;      // at most this many groups of consecutive tiles

// dz of four columns of one row: zhat = (z - mean) rstd, u = zhat g + h, du = act ? dy gelu'(u) : dy,
// dz = (g rstd) (du - mh - zhat mg) with mh = dh / N, mg = dg / N under batch statistics, dz = (g rstd) du otherwise
__device__ __forceinline__ f4 seam_dz4(f4 dy, f4 z, f4 mean, f4 rstd, f4 gam, f4 bet, f4 mh, f4 mg, bool act, bool batch) {
  const f4 zh = (z - mean) * rstd;
  f4 du = dy;
  if (act) {
    const f4 u = zh * gam + bet;
#pragma unroll
    for (int k = 0; k < 4; k++) du[k] = dy[k] * gelu_grad_f(u[k]);
  }
  if (batch) du = du - mh - zh * mg;
  return (gam * rstd) * du;
}
__device__ __forceinline__ f4 seam_act4(f4 z, f4 mean, f4 rstd, f4 gam, f4 bet, bool act) {
  f4 u = ((z - mean) * rstd) * gam + bet;
  if (act) {
#pragma unroll
    for (int k = 0; k < 4; k++) u[k] = gelu_f(u[k]);
  }
  return u;
}
__device__ __forceinline__ f4 seam_rstd4(f4 var, float eps) {
  f4 r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = 1.0f / sqrtf(var[k] + eps);
  return r;
}

// one step of a compensated (Kahan) sum: s + c carries what the float s alone would have rounded away.  The file is built
// without fast-math and without contraction, so the compiler keeps the three subtractions.
__device__ __forceinline__ void kahan_add(float& s, float& c, float x) {
  const float y = x - c, t = s + y;
  c = (t - s) - y;
  s = t;
}

// the tile's column record from its image Zs (rows x columns, pitch zp): thread `col` of the block's first CT.  The mean is
// taken about the tile's first row, mean = z0 + (sum_r (z_r - z0)) / n with a compensated sum, so that neither a column
// whose mean is many standard deviations nor the length of the chain costs digits; M2 is then summed about that mean.
// Both in ascending row order.
__device__ __forceinline__ void seam_tile_record(const float* Zs, int zp, int col, int nv, float* __restrict__ mean,
                                                 float* __restrict__ m2) {
  const float z0 = Zs[col];
  float s = 0.0f, c = 0.0f;
  for (int r = 1; r < nv; r++) kahan_add(s, c, Zs[r * zp + col] - z0);
  const float m = z0 + s / (float)nv;
  float q = 0.0f;
  for (int r = 0; r < nv; r++) {
    const float d = Zs[r * zp + col] - m;
    q += d * d;
  }
  *mean = m;
  *m2 = q;
}

// ---- forward: the product ---------------------------------------------------------------------------------------------
// EVAL: y = act(bn(z)) with the running statistics (mean, var); z and rstd are stored only when asked for.
// !EVAL: z [N][O] contiguous and the tile's records.
template <int NJ, bool EVAL>
__global__ __launch_bounds__(256, 2) void k_seam_forward(const float* __restrict__ x, int64_t xs, const float* __restrict__ w,
                                                         const float* __restrict__ b, const float* __restrict__ mean,
                                                         const float* __restrict__ var, float eps,
                                                         const float* __restrict__ gam, const float* __restrict__ bet, int act,
                                                         int64_t N, int I, int O, float* __restrict__ z, float* __restrict__ y,
                                                         int64_t ys, float* __restrict__ rstd_out, float* __restrict__ part) {
  constexpr int CT = 32 * NJ, XP = kSeamChunk + 4, ZP = CT + 4, CQ = CT / 4;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];       // a chunk of x: rows x inputs; afterwards the tile of z
  __shared__ __attribute__((aligned(16))) float Ws[Chain<NJ, false>::kWords];  // a 16-deep slice of W
  const int tid = threadIdx.x;
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int col0 = blockIdx.y * CT;

  Chain<NJ, false> prod;  // z = x W^T: the accumulators carry across the chunks of inputs
  f4 acc[2][NJ];
  clear_acc(acc);
  for (int i0 = 0; i0 < I; i0 += kSeamChunk) {
    const int cw = I - i0 < kSeamChunk ? I - i0 : kSeamChunk;
    const int Cr = (cw + KC - 1) / KC * KC;
    stage_rows(Xs, XP, Cr >> 2, [&](int r, int c) {
      return (row0 + r < N && i0 + c < I) ? ld4(x + (row0 + r) * xs + i0 + c) : zero4();
    });
    auto w_at = [&](int cl, int k) {
      return (col0 + cl < O && i0 + k < I) ? ld4(w + (int64_t)(col0 + cl) * I + i0 + k) : zero4();
    };
    prod.first(w_at);
    prod.run(acc, g, Xs, XP, Cr, Ws, w_at);
  }

  // z = chain + b into the tile image (the chain's last barrier freed Xs)
  float* Zs = Xs;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int c = col0 + g.first_col<NJ>() + 16 * j + g.fl;
    const float bias = (b && c < O) ? b[c] : 0.0f;
    acc[0][j] = acc[0][j] + bias;
    acc[1][j] = acc[1][j] + bias;
  }
  for_each_output(acc, g, [&](int rl, int cl, float v) { Zs[rl * ZP + cl] = v; });
  __syncthreads();

  for (int e = tid; e < T * CQ; e += 256) {
    const int r = e / CQ, c = col0 + 4 * (e % CQ);
    const int64_t row = row0 + r;
    if (row >= N || c >= O) continue;
    const f4 zv = ld4(&Zs[r * ZP + 4 * (e % CQ)]);
    if (z) st4(z + row * O + c, zv);
    if (EVAL) {
      const f4 rs = seam_rstd4(ld4(var + c), eps);
      st4(y + row * ys + c, seam_act4(zv, ld4(mean + c), rs, ld4(gam + c), ld4(bet + c), act != 0));
      if (rstd_out && row == 0) st4(rstd_out + c, rs);
    }
  }
  if (!EVAL && tid < CT && col0 + tid < O) {
    const int nv = N - row0 < T ? (int)(N - row0) : T;
    float* rec = part + (int64_t)blockIdx.x * 2 * O;
    seam_tile_record(Zs, ZP, tid, nv, rec + col0 + tid, rec + O + col0 + tid);
  }
}

// w == NULL, training: the records of x's tiles; grid (tiles, blocks of 128 columns)
__global__ __launch_bounds__(256) void k_seam_tile_stats(const float* __restrict__ x, int64_t xs, int64_t N, int O,
                                                         float* __restrict__ part) {
  constexpr int CT = kSeamChunk, ZP = CT + 4, CQ = CT / 4;
  __shared__ __attribute__((aligned(16))) float Zs[T * ZP];
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int col0 = blockIdx.y * CT;
  stage_rows(Zs, ZP, CQ, [&](int r, int c) {
    return (row0 + r < N && col0 + c < O) ? ld4(x + (row0 + r) * xs + col0 + c) : zero4();
  });
  __syncthreads();
  if (tid < CT && col0 + tid < O) {
    const int nv = N - row0 < T ? (int)(N - row0) : T;
    float* rec = part + (int64_t)blockIdx.x * 2 * O;
    seam_tile_record(Zs, ZP, tid, nv, rec + col0 + tid, rec + O + col0 + tid);
  }
}

// fn(t, a, b) for the tiles t0 .. t1 in ascending order with a = part[t][0][c], b = part[t][1][c]: the loads of kSeamAhead
// tiles are issued before the first of them is consumed (a thread's walk is a chain of dependent sums; its loads are not)
constexpr int kSeamAhead = 8;
template <typename Fn>
__device__ __forceinline__ void seam_walk_records(const float* __restrict__ part, int O, int c, int64_t t0, int64_t t1, Fn fn) {
  for (int64_t t = t0; t < t1; t += kSeamAhead) {
    float a[kSeamAhead], b[kSeamAhead];
#pragma unroll
    for (int j = 0; j < kSeamAhead; j++) {
      const bool in = t + j < t1;
      a[j] = in ? part[(t + j) * 2 * O + c] : 0.0f;
      b[j] = in ? part[((t + j) * 2 + 1) * O + c] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kSeamAhead; j++)
      if (t + j < t1) fn(t + j, a[j], b[j]);
  }
}

// ---- forward: the statistics --------------------------------------------------------------------------------------------
// 256 threads = 64 groups x 4 columns, two passes over the tiles' records, both in ascending tile order; group q owns its
// gper consecutive tiles, G == 1: one level.  Pass 1: a compensated sum of count_t mean_t per group; every thread of a column
// then adds the groups' sums in ascending order -- the same chain in each, so all hold the same bits -- and the column's
// mean is total / N, one rounding.  Pass 2: M2 = sum_t (M2_t + count_t (mean_t - mean)^2), the deviations taken about that
// FINAL mean, compensated per group and across the groups.  A running (count, mean, M2) merge is not used: its correction
// term (mean_t - running mean)^2 carries the running mean's rounding at first order, tile after tile with one sign, and on
// rows that drift (a serialised point cloud) that put rstd at up to 10.7 x and running_var at up to 40.5 x torch's error
// (262 209 rows); about the final mean those first-order terms cancel (sum_t count_t (mean_t - mean)
// = 0).
__global__ __launch_bounds__(256) void k_seam_stats(const float* __restrict__ part, int64_t tiles, int64_t N, int O, int G,
                                                    int64_t gper, float eps, float momentum, float* __restrict__ mean,
                                                    float* __restrict__ rstd, float* __restrict__ rmean,
                                                    float* __restrict__ rvar, int64_t* __restrict__ tracked) {
  __shared__ float Ss[kSeamGroups][4], Sc[kSeamGroups][4], Sq[kSeamGroups][4], Sd[kSeamGroups][4];
  const int q = threadIdx.x >> 2, cl = threadIdx.x & 3, c = blockIdx.x * 4 + cl;
  const bool own = q < G && c < O;
  const int64_t t0 = q * gper, t1 = t0 + gper < tiles ? t0 + gper : tiles;
  auto count = [&](int64_t t) { return (float)(N - t * T < T ? N - t * T : T); };
  float sum = 0.0f, comp = 0.0f;
  if (own) seam_walk_records(part, O, c, t0, t1, [&](int64_t t, float mt, float) { kahan_add(sum, comp, count(t) * mt); });
  Ss[q][cl] = sum;
  Sc[q][cl] = comp;
  __syncthreads();
  sum = Ss[0][cl];
  comp = Sc[0][cl];
  for (int k = 1; k < G; k++) {
    kahan_add(sum, comp, Ss[k][cl]);
    kahan_add(sum, comp, -Sc[k][cl]);
  }
  const float m = (sum - comp) / (float)N;
  float m2 = 0.0f, mc = 0.0f;
  if (own)
    seam_walk_records(part, O, c, t0, t1, [&](int64_t t, float mt, float qt) {
      const float d = mt - m;
      kahan_add(m2, mc, qt);
      kahan_add(m2, mc, count(t) * (d * d));
    });
  Sq[q][cl] = m2;
  Sd[q][cl] = mc;
  __syncthreads();
  if (q != 0 || c >= O) return;
  for (int k = 1; k < G; k++) {
    kahan_add(m2, mc, Sq[k][cl]);
    kahan_add(m2, mc, -Sd[k][cl]);
  }
  m2 -= mc;
  mean[c] = m;
  rstd[c] = 1.0f / sqrtf(m2 / (float)N + eps);
  if (rmean) {  // one thread per column, plain stores
    rmean[c] = (1.0f - momentum) * rmean[c] + momentum * m;
    rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (m2 / (float)(N - 1));
    if (c == 0) tracked[0] += 1;
  }
}

// ---- forward: apply ------------------------------------------------------------------------------------------------------
// one thread per 16 bytes of y; o4 = O / 4.  FROM_VAR: `spread` is a variance (eval, w == NULL), else it is rstd.
template <bool FROM_VAR>
__global__ __launch_bounds__(256) void k_seam_apply(const float* __restrict__ z, int64_t zs, const float* __restrict__ mean,
                                                    const float* __restrict__ spread, float eps,
                                                    const float* __restrict__ gam, const float* __restrict__ bet, int act,
                                                    int64_t N, int o4, float* __restrict__ y, int64_t ys,
                                                    float* __restrict__ rstd_out) {
  const int64_t base = (int64_t)blockIdx.x * 256, r0 = base / o4;  // uniform: one wide division per wave
  const unsigned local = (unsigned)(base - r0 * o4) + threadIdx.x;
  const int64_t r = r0 + local / (unsigned)o4;
  const int c = 4 * (int)(local % (unsigned)o4);
  if (r >= N) return;
  const f4 rs = FROM_VAR ? seam_rstd4(ld4(spread + c), eps) : ld4(spread + c);
  st4(y + r * ys + c, seam_act4(ld4(z + r * zs + c), ld4(mean + c), rs, ld4(gam + c), ld4(bet + c), act != 0));
  if (FROM_VAR && rstd_out && r == 0) st4(rstd_out + c, rs);
}

// ---- backward: dh, dg -----------------------------------------------------------------------------------------------------
// grid (tiles, blocks of 64 columns); thread = (16 rows, column); a tile's record [2][O] = dh, dg
__global__ __launch_bounds__(256) void k_seam_bwd_part(const float* __restrict__ dy, int64_t dys, const float* __restrict__ z,
                                                       int64_t zs, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gam,
                                                       const float* __restrict__ bet, int act, int64_t N, int O,
                                                       float* __restrict__ part) {
  __shared__ float Sh[4][T], Sg[4][T];
  const int cl = threadIdx.x & 63, rq = threadIdx.x >> 6, c = blockIdx.y * T + cl;
  const int64_t row0 = (int64_t)blockIdx.x * T + 16 * rq;
  float sh = 0.0f, sg = 0.0f;
  if (c < O) {
    const float mu = mean[c], rs = rstd[c], ga = gam[c], be = bet[c];
    for (int k = 0; k < 16; k++) {
      const int64_t r = row0 + k;
      if (r >= N) break;
      const float zh = (z[r * zs + c] - mu) * rs;
      float du = dy[r * dys + c];
      if (act) du = du * gelu_grad_f(zh * ga + be);
      sh += du;
      sg += du * zh;
    }
  }
  Sh[rq][cl] = sh;
  Sg[rq][cl] = sg;
  __syncthreads();
  if (rq == 0 && c < O) {
    float* rec = part + (int64_t)blockIdx.x * 2 * O;
    rec[c] = ((Sh[0][cl] + Sh[1][cl]) + Sh[2][cl]) + Sh[3][cl];
    rec[O + c] = ((Sg[0][cl] + Sg[1][cl]) + Sg[2][cl]) + Sg[3][cl];
  }
}

// k_seam_stats' layout; compensated sums in the same fixed order (plain sums over 4098 tiles had dbn_b at 5.35 x torch's
// figure); `keep` [2][O] = dh, dg for the kernels that form dz
__global__ __launch_bounds__(256) void k_seam_bwd_fold(const float* __restrict__ part, int64_t tiles, int O, int G,
                                                       int64_t gper, float* __restrict__ dg, float* __restrict__ dh,
                                                       float* __restrict__ keep) {
  __shared__ float Sh[kSeamGroups][4], Sg[kSeamGroups][4], Ch[kSeamGroups][4], Cg[kSeamGroups][4];
  const int q = threadIdx.x >> 2, cl = threadIdx.x & 3, c = blockIdx.x * 4 + cl;
  float sh = 0.0f, sg = 0.0f, ch = 0.0f, cg = 0.0f;
  if (q < G && c < O) {
    const int64_t t0 = q * gper, t1 = t0 + gper < tiles ? t0 + gper : tiles;
    seam_walk_records(part, O, c, t0, t1, [&](int64_t, float ht, float gt) {
      kahan_add(sh, ch, ht);
      kahan_add(sg, cg, gt);
    });
  }
  Sh[q][cl] = sh;
  Sg[q][cl] = sg;
  Ch[q][cl] = ch;
  Cg[q][cl] = cg;
  __syncthreads();
  if (q != 0 || c >= O) return;
  for (int k = 1; k < G; k++) {
    kahan_add(sh, ch, Sh[k][cl]);
    kahan_add(sh, ch, -Ch[k][cl]);
    kahan_add(sg, cg, Sg[k][cl]);
    kahan_add(sg, cg, -Cg[k][cl]);
  }
  sh -= ch;
  sg -= cg;
  if (dh) dh[c] = sh;
  if (dg) dg[c] = sg;
  keep[c] = sh;
  keep[O + c] = sg;
}

// what the kernels that form dz share; kh, kg: dh and dg [O], both NULL under running statistics
struct SeamDz {
  const float *dy, *z, *mean, *rstd, *gam, *bet, *kh, *kg;
  int64_t dys, zs;
  float inv_n;
  int act;
  __device__ __forceinline__ f4 at(int64_t r, int c) const {
    f4 mh = zero4(), mg = zero4();
    if (kh) {
      mh = ld4(kh + c) * inv_n;
      mg = ld4(kg + c) * inv_n;
    }
    return seam_dz4(ld4(dy + r * dys + c), ld4(z + r * zs + c), ld4(mean + c), ld4(rstd + c), ld4(gam + c), ld4(bet + c), mh,
                    mg, act != 0, kh != nullptr);
  }
};

// ---- backward: dx ---------------------------------------------------------------------------------------------------------
// w == NULL: dx is dz; one thread per 16 bytes, o4 = O / 4
__global__ __launch_bounds__(256) void k_seam_dz(SeamDz d, int64_t N, int o4, float* __restrict__ dx, int64_t dxs) {
  const int64_t base = (int64_t)blockIdx.x * 256, r0 = base / o4;
  const unsigned local = (unsigned)(base - r0 * o4) + threadIdx.x;
  const int64_t r = r0 + local / (unsigned)o4;
  const int c = 4 * (int)(local % (unsigned)o4);
  if (r >= N) return;
  st4(dx + r * dxs + c, d.at(r, c));
}

// 256 threads own T = 64 rows and CT = 32 NJ columns of dx (grid.y walks I); the outputs are the
// summed index, walked in chunks of <= 128 of dz staged in LDS.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_seam_dx(SeamDz d, const float* __restrict__ w, int64_t N, int I, int O,
                                                    float* __restrict__ dx, int64_t dxs) {
  constexpr int CT = 32 * NJ, XP = kSeamChunk + 4;
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];                   // dz: rows x a chunk of outputs
  __shared__ __attribute__((aligned(16))) float Ws[Chain<NJ, true>::kWords];  // a 16-deep slice of W
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int col0 = blockIdx.y * CT;

  Chain<NJ, true> back;  // dx = dz W, a chain per chunk of outputs
  f4 acc[2][NJ], tot[2][NJ];
  clear_acc(tot);
  for (int o0 = 0; o0 < O; o0 += kSeamChunk) {
    const int cw = O - o0 < kSeamChunk ? O - o0 : kSeamChunk;
    const int Cr = (cw + KC - 1) / KC * KC;
    stage_rows(Ds, XP, Cr >> 2, [&](int r, int c) { return (row0 + r < N && o0 + c < O) ? d.at(row0 + r, o0 + c) : zero4(); });
    auto w_at = [&](int cl, int k) {
      return (o0 + k < O && col0 + cl < I) ? ld4(w + (int64_t)(o0 + k) * I + col0 + cl) : zero4();
    };
    clear_acc(acc);
    back.first(w_at);
    back.run(acc, g, Ds, XP, Cr, Ws, w_at);
    add_acc(tot, acc);
  }
  for_each_output(tot, g, [&](int rl, int cl, float v) {
    const int64_t row = row0 + rl;
    if (row < N && col0 + cl < I) dx[row * dxs + col0 + cl] = v;
  });
}

// ---- backward: the weight gradient ----------------------------------------------------------------------------------------
// A slice's record in `part`: dW [O][I], db [O].
__host__ __device__ inline int64_t seam_record(int I, int O) { return (int64_t)O * I + O; }

// grid: (tiles of 64 x 64 over O x I, row slices): dW[o][i] = sum_r dz[r][o] x[r][i], db[o] = sum_r dz[r][o]
__global__ __launch_bounds__(256) void k_seam_dw(SeamDz d, const float* __restrict__ x, int64_t xs, int64_t N, int I, int O,
                                                 int64_t per, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ds[KC * kPitchT];
  __shared__ __attribute__((aligned(16))) float Xs[KC * kPitchT];
  float* rec = part + (int64_t)blockIdx.y * seam_record(I, O);
  const int tiles_i = (I + T - 1) / T;
  const int o0 = (blockIdx.x / tiles_i) * T, i0 = (blockIdx.x % tiles_i) * T;
  const int64_t p0 = blockIdx.y * per, p1 = p0 + per < N ? p0 + per : N;
  const int sc = 4 * (threadIdx.x & 15);
  auto fetch = [&](int64_t r, bool od, bool ix, f4& vd, f4& vx) {
    if (od) vd = d.at(r, o0 + sc);
    if (ix) vx = ld4(x + r * xs + i0 + sc);
  };
  dw_slice_tile(fetch, O, I, o0, i0, p0, p1, rec, rec + (int64_t)O * I, Ds, Xs);
}

// ---- host: the plans -----------------------------------------------------------------------------------
struct SeamPlan {
  int64_t tiles;  // row tiles
  int G;          // groups of consecutive tiles (1: one level)
  int64_t gper;   // tiles per group
  int sw;         // row slices of the weight gradient
  unsigned wt;    // 64 x 64 tiles of the weight gradient
  size_t part, keep, wpart, total;  // backward; the forward's workspace is `part` alone
};
SeamPlan seam_plan(int64_t N, int32_t I, int32_t O) {
  SeamPlan p;
  p.tiles = (N + T - 1) / T;
  p.G = p.tiles > kSeamFoldTiles ? (int)std::min<int64_t>(kSeamGroups, (p.tiles + kSeamFoldTiles - 1) / kSeamFoldTiles) : 1;
  p.gper = (p.tiles + p.G - 1) / p.G;
  p.wt = (unsigned)((O + T - 1) / T) * (unsigned)((I + T - 1) / T);
  p.sw = weight_slices(p.wt, N);
  Carve ws;
  p.part = ws.take((size_t)std::max<int64_t>(p.tiles, 1) * 2 * O * 4);
  p.keep = ws.take((size_t)2 * O * 4);
  p.wpart = ws.take((size_t)p.sw * (size_t)seam_record(I, O) * 4);
  p.total = ws.off;
  return p;
}
size_t seam_forward_bytes(int64_t N, int32_t O) { return seam_plan(N, 4, O).keep; }  // the tiles' records, rounded

}  // namespace
