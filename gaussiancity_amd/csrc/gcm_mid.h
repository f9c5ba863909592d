// gcm_mid.h -- the middle of a PTv3 Block around its attention (gcm_mid_*, include/gcm.h): the gather of the projected rows
// into patch order, and, after the attention, the scatter back to point order, the output projection, DropPath and the
// residual add in ONE launch; the deterministic backward of both in two or three launches whatever N is.  Included by
// gcm_modlinear.hip after gcm_tile.h (the tile and the product loop) and gcm_ffn.h (the row-sliced weight gradient); device
// code and the plan only, the C ABI stays in gcm_modlinear.hip.  DESIGN.md section 20.
//
// The two index vectors: order [T] (slot -> row, T >= N, one entry per padded slot) and inverse [N] (row -> its own slot),
// with order[inverse[n]] == n.  A slot j with inverse[order[j]] != j is a duplicate slot; a row has at most one, extra[n]
// (-1: none), which k_mid_slot_plan finds.  Under that precondition every sum below has at most two terms and every
// output element one writer:
//   gather forward    y[j] = x[order[j]]
//   gather backward   dx[n] = dy[inverse[n]] (+ dy[extra[n]]), one fp32 add
//   forward           a[inverse[n]] tile -> LDS; p = a Wp^T (one chain over C) + bp; y = x + p, or x + (p r[n])
//   backward          k_mid_bwd_rows: g = r o dy -> LDS, da[inverse[n]] = g Wp (one chain over C), da[extra[n]] = 0;
//                     k_mid_dw: dWp = g^T a[inverse] in row slices (dw_slice_tile, gathered loads), dbp the column sums of
//                     the slice's g; k_ffn_fold_params adds the slices pairwise, a fixed tree.
// An index outside its range is never dereferenced where the range is known: the row is skipped (zeros are staged).
#pragma once

namespace {

constexpr int kMidMaxChannels = kFfnMaxChannels;  // widest instantiation (NJ = 4)

// ---- the slot plan ------------------------------------------------------------------------------------------------------
__global__ void k_mid_fill(int32_t* __restrict__ extra, int64_t N) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) extra[n] = -1;
}
// one thread per slot: the slot of a row that is not the row's own is its duplicate slot (one writer under the precondition)
__global__ void k_mid_slot_plan(const int64_t* __restrict__ order, int64_t Tn, const int64_t* __restrict__ inverse, int64_t N,
                                int32_t* __restrict__ extra) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Tn) return;
  const int64_t n = order[j];
  if (n < 0 || n >= N) return;
  if (inverse[n] != j) extra[n] = (int32_t)j;
}

// ---- the gather and its gradient ------------------------------------------------------------------------------------------
// one thread per 16 bytes of the output; w4 = W / 4
__global__ __launch_bounds__(256) void k_mid_gather_forward(const float* __restrict__ x, int64_t xs,
                                                            const int64_t* __restrict__ order, int64_t Tn, int w4,
                                                            float* __restrict__ y) {
  const int64_t base = (int64_t)blockIdx.x * 256, j0 = base / w4;  // uniform: one wide division per wave
  const unsigned local = (unsigned)(base - j0 * w4) + threadIdx.x;
  const int64_t j = j0 + local / (unsigned)w4;
  const int c = 4 * (int)(local % (unsigned)w4);
  if (j >= Tn) return;
  const int64_t n = order[j];
  st4(y + j * 4 * w4 + c, n >= 0 ? ld4(x + n * xs + c) : zero4());
}
__global__ __launch_bounds__(256) void k_mid_gather_backward(const float* __restrict__ dy, int64_t dys,
                                                             const int64_t* __restrict__ inverse,
                                                             const int32_t* __restrict__ extra, int64_t N, int w4,
                                                             float* __restrict__ dx) {
  const int64_t base = (int64_t)blockIdx.x * 256, n0 = base / w4;
  const unsigned local = (unsigned)(base - n0 * w4) + threadIdx.x;
  const int64_t n = n0 + local / (unsigned)w4;
  const int c = 4 * (int)(local % (unsigned)w4);
  if (n >= N) return;
  const int64_t j = inverse[n];
  const int32_t k = extra[n];
  f4 v = j >= 0 ? ld4(dy + j * dys + c) : zero4();
  if (k >= 0) v = v + ld4(dy + (int64_t)k * dys + c);
  st4(dx + n * 4 * w4 + c, v);
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// 256 threads own T = 64 rows and CT = 32 NJ channels.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_mid_forward(const float* __restrict__ a, int64_t as, const int64_t* __restrict__ inverse,
                                                        const float* __restrict__ x, int64_t xs, const float* __restrict__ wp,
                                                        const float* __restrict__ bp, const float* __restrict__ rscale,
                                                        int64_t N, int C, float* __restrict__ y, int64_t ys) {
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Xs[T * XP];                      // a[inverse]: rows x channels
  __shared__ __attribute__((aligned(16))) float Ws[(CT > T ? CT : T) * kPitch];  // a 16-deep slice of Wp
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC;

  stage_rows(Xs, XP, Cr >> 2, [&](int r, int c) {
    f4 v = zero4();
    if (row0 + r < N && c < C) {
      const int64_t j = inverse[row0 + r];
      if (j >= 0) v = ld4(a + j * as + c);
    }
    return v;
  });

  Chain<NJ, false> proj;  // p = a Wp^T
  auto wp_at = [&](int c, int k) { return (c < C && k < C) ? ld4(wp + (int64_t)c * C + k) : zero4(); };
  f4 acc[2][NJ];
  clear_acc(acc);
  proj.first(wp_at);
  proj.run(acc, g, Xs, XP, Cr, Ws, wp_at);

  // p = chain + bp; y = x + p, or x + (p r): a multiply, then an add (the file is built without contraction)
  for_each_output(
      acc, g, [&](int rl) { return scaled_row(row0 + rl, N, rscale); },
      [&](ScaledRow r, int c, float v) {
        if (r.row < 0 || c >= C) return;
        const float p = v + bp[c];
        y[r.row * ys + c] = x[r.row * xs + c] + (rscale ? p * r.scale : p);
      });
}

// ---- backward, the row tiles --------------------------------------------------------------------------------------------
// da [Tn][C]: row inverse[n] = (r[n] dy[n]) Wp, row extra[n] = 0, both written by the workgroup that owns n.
template <int NJ>
__global__ __launch_bounds__(256, 2) void k_mid_bwd_rows(const float* __restrict__ dy, int64_t dys,
                                                         const int64_t* __restrict__ inverse,
                                                         const int32_t* __restrict__ extra, const float* __restrict__ wp,
                                                         const float* __restrict__ rscale, int64_t N, int64_t Tn, int C,
                                                         float* __restrict__ da) {
  constexpr int CT = 32 * NJ, XP = CT + 4;
  __shared__ __attribute__((aligned(16))) float Ds[T * XP];                   // g = r o dy: rows x channels
  __shared__ __attribute__((aligned(16))) float Ws[Chain<NJ, true>::kWords];  // a 16-deep slice of Wp
  const int tid = threadIdx.x;
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int Cr = (C + KC - 1) / KC * KC;

  stage_rows(Ds, XP, Cr >> 2, [&](int r, int c) {
    f4 v = zero4();
    if (row0 + r < N && c < C) {
      v = ld4(dy + (row0 + r) * dys + c);
      if (rscale) v = v * rscale[row0 + r];
    }
    return v;
  });
  {  // the duplicate slots of the tile's rows: exact zeros, four lanes per row
    const int r = tid >> 2, q = tid & 3;
    if (row0 + r < N) {
      const int64_t k = extra[row0 + r];
      if (k >= 0 && k < Tn)
        for (int c = 4 * q; c < C; c += 16) st4(da + k * C + c, zero4());
    }
  }

  Chain<NJ, true> back;  // da = g Wp
  auto wp_at = [&](int c, int k) { return (k < C && c < C) ? ld4(wp + (int64_t)k * C + c) : zero4(); };
  f4 acc[2][NJ];
  clear_acc(acc);
  back.first(wp_at);
  back.run(acc, g, Ds, XP, Cr, Ws, wp_at);
  for_each_output(
      acc, g,
      [&](int rl) -> int64_t {  // the row's slot, -1 without one
        if (row0 + rl >= N) return -1;
        const int64_t slot = inverse[row0 + rl];
        return slot < Tn ? slot : -1;
      },
      [&](int64_t slot, int c, float v) {
        if (slot >= 0 && c < C) da[slot * C + c] = v;
      });
}

// ---- backward, the weight gradient ----------------------------------------------------------------------------------------
// A slice's record in `part`: dWp [C][C], dbp [C].
__host__ __device__ inline int64_t mid_record(int C) { return (int64_t)C * C + C; }

// grid: (tiles of 64 x 64 over C x C, row slices): dWp[o][c] = sum_n g[n][o] a[inverse[n]][c], dbp[o] = sum_n g[n][o]
__global__ __launch_bounds__(256) void k_mid_dw(const float* __restrict__ a, int64_t as, const int64_t* __restrict__ inverse,
                                                const float* __restrict__ dy, int64_t dys, const float* __restrict__ rscale,
                                                int64_t N, int64_t Tn, int C, int64_t per, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Ds[KC * kPitchT];
  __shared__ __attribute__((aligned(16))) float Xs[KC * kPitchT];
  float* rec = part + (int64_t)blockIdx.y * mid_record(C);
  const int tiles_i = (C + T - 1) / T;
  const int o0 = (blockIdx.x / tiles_i) * T, i0 = (blockIdx.x % tiles_i) * T;
  const int64_t p0 = blockIdx.y * per, p1 = p0 + per < N ? p0 + per : N;
  const int sc = 4 * (threadIdx.x & 15);
  auto fetch = [&](int64_t r, bool od, bool ix, f4& vd, f4& vx) {
    if (od) {
      vd = ld4(dy + r * dys + o0 + sc);
      if (rscale) vd = vd * rscale[r];
    }
    if (ix) {
      const int64_t j = inverse[r];
      if (j >= 0 && j < Tn) vx = ld4(a + j * as + i0 + sc);
    }
  };
  dw_slice_tile(fetch, C, C, o0, i0, p0, p1, rec, rec + (int64_t)C * C, Ds, Xs);
}

// ---- host: the plan ------------------------------------------------------------------------------------
struct MidPlan {
  int64_t tiles;  // row tiles
  int sw;         // row slices of the weight gradient
  unsigned wt;    // 64 x 64 tiles of the weight gradient
  size_t total;    // the slices' records
};
MidPlan mid_plan(int64_t N, int32_t C) {
  MidPlan p;
  p.tiles = (N + T - 1) / T;
  p.wt = (unsigned)((C + T - 1) / T) * (unsigned)((C + T - 1) / T);
  p.sw = weight_slices(p.wt, N);
  p.total = round256((size_t)p.sw * (size_t)mid_record(C) * 4);
  return p;
}

}  // namespace
