// gcm_tile.h -- what the row-tile operators of libgcm_hip.so share (gcm_ffn.h, gcm_front.h, gcm_mid.h, gcm_seam.h and the
// attribute head in gcm_modlinear.hip, which includes this file first): the 64-row workgroup tile, its accumulators, the
// ONE product loop on v_mfma_f32_16x16x4_f32 in its two forms, the tile staging loop, the LayerNorm over a row's four
// lanes both ways with its column sums, and the host rules every plan repeats.  Device code is __forceinline__ and takes
// its per-operator parts as callables; nothing is called through a pointer.  DESIGN.md section 17a.  (gcm_chain.h, the
// attribute head in one launch, takes the constants, the accumulators and the epilogue nest from here and runs Chain's loop
// written out for its 512 threads.)
//
// The tile.  A workgroup of 256 threads (4 waves as 2 x 2) owns T = 64 rows; a wave owns 32 rows x 16 J columns as
// f4 acc[2][J] (C/D layout of the MFMA: column = lane & 15, row = 4 * (lane >> 4) + register), J = 1, 2 or 4, its first
// column wcn = 16 J * (wave & 1).  The rows live in LDS as an image "rows x summed index"; the weights come through LDS
// in slices KC = 16 deep.
//
// The product loop (Chain::run).  Per slice: put the slice from the staging registers into LDS; barrier; issue the global
// loads of the next slice into the registers (they land under the MFMAs); four MFMA steps per accumulator against the
// row image; barrier.  The first barrier orders the put -- and whatever the caller wrote to the row image before the
// chain -- before the fragment reads; the second keeps the next put, and whatever the caller writes to either image
// after the chain, behind the last fragment read.  So a caller needs no barrier of its own between staging rows and
// running a chain, nor between a chain and overwriting its images.  first() loads slice 0; a caller may issue it early,
// from the tail callable of the chain before: run() calls tail() in its last slice, where there is no next slice to
// fetch.  An accumulator is one fp32 chain over the summed index in ascending order; run() never clears it.
//   N-form (TFORM = false)  weight read as w[column][k], slice image Ws[column][k] at kPitch: forward products.
//   T-form (TFORM = true)   weight read as w[k][column], slice image Ws[k][column] at 32 J + 16: products with W itself.
// w_at(column, k) returns four consecutive weights -- along k in the N-form, along the columns in the T-form -- or zeros
// out of range; column counts from the workgroup's first column, k from the start of the chain.
//
// The lane rule of the LayerNorms.  Four lanes per row, lane q owns the elements 4 q + 16 k .. + 3: one chain per lane in
// element order (sum4), then quad_sum over the four lanes, which leaves the same bits in all four.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int KC = 16;            // depth of a staged slice
constexpr int T = 64;             // workgroup tile, both ways
constexpr int kPitch = KC + 4;    // words between rows of an image that holds the summed index contiguously
constexpr int kPitchT = T + 16;   // words between rows of an image that holds the summed index in rows
constexpr int FH = 64;            // features per chunk of the operators that walk a second width
constexpr int kPitchG = FH + 4;   // words between rows of a chunk image (rows x features)

__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
__device__ __forceinline__ f4 zero4() { return f4{0.0f, 0.0f, 0.0f, 0.0f}; }

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

struct WaveTile {  // wave (wr, wc): tile-relative corner of the wave's 32 x 32 outputs; (fl, fk): the lane in a fragment
  int wr, wc, fl, fk;
  __device__ __forceinline__ WaveTile() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wr = (wave >> 1) * 32;
    wc = (wave & 1) * 32;
    fl = lane & 15;
    fk = lane >> 4;
  }
  template <int J>
  __device__ __forceinline__ int first_col() const { return (wc >> 5) * 16 * J; }  // wc itself for J = 2
};

// ---- accumulators -------------------------------------------------------------------------------------------------------
template <int J>
__device__ __forceinline__ void clear_acc(f4 (&acc)[2][J]) {
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < J; j++) acc[i][j] = zero4();
}
template <int J>
__device__ __forceinline__ void add_acc(f4 (&tot)[2][J], const f4 (&acc)[2][J]) {  // tot += acc
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < J; j++) tot[i][j] = tot[i][j] + acc[i][j];
}
// The epilogue nest: fn(row(rl), cl, value) for each of the lane's 8 J outputs, rl the row in the tile, cl the column from
// the workgroup's first.  row(rl) runs once per row, before the row's J outputs: what a row loads (its scale, its slot)
// belongs there -- a load under a test is not hoisted out of fn by the compiler.  Without it fn gets rl itself.
template <int J, typename Row, typename Fn>
__device__ __forceinline__ void for_each_output(const f4 (&acc)[2][J], const WaveTile& g, Row row, Fn fn) {
  const int wcn = g.first_col<J>();
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const auto r = row(g.wr + 16 * i + 4 * g.fk + v);
#pragma unroll
      for (int j = 0; j < J; j++) fn(r, wcn + 16 * j + g.fl, acc[i][j][v]);
    }
}
template <int J, typename Fn>
__device__ __forceinline__ void for_each_output(const f4 (&acc)[2][J], const WaveTile& g, Fn fn) {
  for_each_output(acc, g, [](int rl) { return rl; }, fn);
}

// a row of the tile in the tensor and its scale (DropPath's mask; 1 without one); row -1: beyond N
struct ScaledRow {
  int64_t row;
  float scale;
};
__device__ __forceinline__ ScaledRow scaled_row(int64_t row, int64_t N, const float* __restrict__ s) {
  if (row >= N) return {-1, 1.0f};
  return {row, s ? s[row] : 1.0f};
}

// ---- the product loop ---------------------------------------------------------------------------------------------------
struct NoTail {
  __device__ __forceinline__ void operator()() const {}
};

template <int J, bool TFORM>
struct Chain {
  static constexpr int CT = 32 * J;                       // columns of the slice
  static constexpr int WP = TFORM ? CT + 16 : kPitch;     // words between rows of the slice image
  static constexpr int PER = TFORM ? CT / 4 : KC / 4;     // f4 pieces per row of the slice image
  static constexpr int PIECES = KC * CT / 4, NV = (PIECES + 255) / 256;
  static constexpr bool kWhole = PIECES % 256 == 0;  // every one of the 256 threads has a piece in every round (J = 2, 4)
  static constexpr int kWords = TFORM ? KC * WP : CT * WP;  // what Ws must hold
  f4 vw[NV];  // the slice in flight

  template <typename W>
  __device__ __forceinline__ void fetch(W w_at, int k0) {
#pragma unroll
    for (int u = 0; u < NV; u++) {
      const int e = threadIdx.x + 256 * u, row = e / PER, piece = 4 * (e % PER);
      vw[u] = (kWhole || e < PIECES) ? (TFORM ? w_at(piece, k0 + row) : w_at(row, k0 + piece)) : zero4();
    }
  }
  template <typename W>
  __device__ __forceinline__ void first(W w_at) { fetch(w_at, 0); }

  // acc += X[rows][0 .. kext) . W over the chain's kext summed indices (a multiple of KC); X: the row image, pitch xp
  template <int WN, typename W, typename Tail = NoTail>
  __device__ __forceinline__ void run(f4 (&acc)[2][J], const WaveTile& g, const float* X, int xp, int kext, float (&Ws)[WN],
                                      W w_at, Tail tail = Tail()) {
    static_assert(WN >= kWords, "the slice buffer holds a 16-deep slice of 32 J columns");
    const int wcn = g.first_col<J>();
    for (int k0 = 0; k0 < kext; k0 += KC) {
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const int e = threadIdx.x + 256 * u;
        if (kWhole || e < PIECES) st4(&Ws[(e / PER) * WP + 4 * (e % PER)], vw[u]);
      }
      __syncthreads();
      if (k0 + KC < kext) fetch(w_at, k0 + KC);
      else tail();
#pragma unroll
      for (int kk = 0; kk < KC; kk += 4) {
        float fa[2], fb[J];
#pragma unroll
        for (int i = 0; i < 2; i++) fa[i] = X[(g.wr + 16 * i + g.fl) * xp + k0 + kk + g.fk];
#pragma unroll
        for (int j = 0; j < J; j++)
          fb[j] = TFORM ? Ws[(kk + g.fk) * WP + wcn + 16 * j + g.fl] : Ws[(wcn + 16 * j + g.fl) * WP + kk + g.fk];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
          for (int j = 0; j < J; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
};

// ---- staging a tile -------------------------------------------------------------------------------------------------------
// image[r][4 c4' .. + 3] = fn(r, 4 c4') for the tile's T rows and c4 pieces a row
template <typename Fn>
__device__ __forceinline__ void stage_rows(float* image, int pitch, int c4, Fn fn) {
  for (int e = threadIdx.x; e < T * c4; e += 256) {
    const int r = e / c4, c = 4 * (e % c4);
    st4(&image[r * pitch + c], fn(r, c));
  }
}

// ---- LayerNorm over a row's four lanes ------------------------------------------------------------------------------------
struct RowStat {
  float mean, rstd;
};
// The lane's share of row Xr (C elements in LDS): each(c, v) sees every element while it is summed, then the row's mean
// and rstd, then Xr[c] = out(c, (v - mean) rstd).  A lane reads and writes its own elements only.
template <typename Each, typename Out>
__device__ __forceinline__ RowStat ln_rows_forward(float* Xr, int q, int C, float eps, Each each, Out out) {
  float sum = 0.0f;
  for (int c = 4 * q; c < C; c += 16) {
    const f4 v = ld4(&Xr[c]);
    sum = sum4(sum, v);
    each(c, v);
  }
  const float mu = quad_sum(sum) / (float)C;
  float sq = 0.0f;
  for (int c = 4 * q; c < C; c += 16) {
    const f4 d = ld4(&Xr[c]) - mu;
    sq = sum4(sq, d * d);
  }
  const float rs = 1.0f / sqrtf(quad_sum(sq) / (float)C + eps);
  for (int c = 4 * q; c < C; c += 16) {
    const f4 d = ld4(&Xr[c]) - mu;
    st4(&Xr[c], out(c, d * rs));
  }
  return {mu, rs};
}

// The backward of h = (src - mean) rstd, y = h gamma for the lane's share of a row: u = Dr gamma (Dr: dy in LDS),
// out(c, rstd (u - mean_c(u) - h mean_c(u h))) for the live elements (live && c < C), rest(c) for the others the
// instantiation holds.  src(c): the four inputs at c.
template <int NJ, typename Src, typename Out, typename Rest>
__device__ __forceinline__ void ln_rows_backward(const float* Dr, int q, int C, bool live, RowStat st,
                                                 const float* __restrict__ gamma, Src src, Out out, Rest rest) {
  f4 h[2 * NJ], wd[2 * NJ];
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 2 * NJ; k++) {
    const int c = 4 * q + 16 * k;
    h[k] = zero4();
    wd[k] = zero4();
    if (live && c < C) {
      h[k] = (src(c) - st.mean) * st.rstd;
      wd[k] = ld4(&Dr[c]) * ld4(gamma + c);
      s1 = sum4(s1, wd[k]);
      s2 = sum4(s2, wd[k] * h[k]);
    }
  }
  const float c1 = quad_sum(s1) / (float)C, c2 = quad_sum(s2) / (float)C;
#pragma unroll
  for (int k = 0; k < 2 * NJ; k++) {
    const int c = 4 * q + 16 * k;
    if (live && c < C) out(c, (wd[k] - c1 - h[k] * c2) * st.rstd);
    else rest(c);
  }
}

// The same for widths whose 2 NJ register pairs would not fit (CT = 256, 512): h and u are formed twice, from the same
// loads by the same operations, so every value and each lane's two sums (element order) are those of the form above.
template <typename Src, typename Out>
__device__ __forceinline__ void ln_rows_backward_reread(const float* Dr, int q, int C, bool live, RowStat st,
                                                        const float* __restrict__ gamma, Src src, Out out) {
  float s1 = 0.0f, s2 = 0.0f;
  if (live)
    for (int c = 4 * q; c < C; c += 16) {
      const f4 h = (src(c) - st.mean) * st.rstd, wd = ld4(&Dr[c]) * ld4(gamma + c);
      s1 = sum4(s1, wd);
      s2 = sum4(s2, wd * h);
    }
  const float c1 = quad_sum(s1) / (float)C, c2 = quad_sum(s2) / (float)C;
  if (live)
    for (int c = 4 * q; c < C; c += 16) {
      const f4 h = (src(c) - st.mean) * st.rstd, wd = ld4(&Dr[c]) * ld4(gamma + c);
      out(c, (wd - c1 - h * c2) * st.rstd);
    }
}

// out[0][c] = sum_r d[r][c] h[r][c], out[1][c] = sum_r d[r][c] over the tile's live rows, d the LDS image Ds (pitch CT + 4)
// and h = (src - mean) rstd read per row: thread (row group, f4 column) sums its RPG rows in order, then the groups in
// order.  Gs (a chunk image) holds the groups' partials; the caller keeps a __syncthreads between two calls.
template <int CT>
__device__ __forceinline__ void ln_col_sums(const float* Ds, const float* __restrict__ src, int64_t ss, const float* sMean,
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
        const f4 d = ld4(&Ds[r * XP + c]);
        const f4 h = (ld4(src + (row0 + r) * ss + c) - sMean[r]) * sRstd[r];
        pg = pg + d * h;
        pb = pb + d;
      }
    }
    st4(&Gs[(grp * 2 + 0) * CT + c], pg);
    st4(&Gs[(grp * 2 + 1) * CT + c], pb);
  }
  __syncthreads();
  for (int e = tid; e < 2 * CT; e += 256) {  // one round up to CT = 128
    const int which = e / CT, c = e % CT;
    if (c < C) {
      float v = Gs[which * CT + c];
      for (int grp = 1; grp < GROUPS; grp++) v += Gs[(grp * 2 + which) * CT + c];
      out[which * C + c] = v;
    }
  }
}

// ---- folding the tiles' LayerNorm partials --------------------------------------------------------------------------------
// out[q][e] = sum of part[s][e] over the `per` records of group q (blockIdx.y), s ascending
__global__ void k_ffn_fold_groups(const float* __restrict__ part, int64_t S, int len, int64_t per, float* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  const int64_t s0 = blockIdx.y * per, s1 = s0 + per < S ? s0 + per : S;
  float v = 0.0f;
  for (int64_t s = s0; s < s1; s++) v += part[s * len + e];
  out[(int64_t)blockIdx.y * len + e] = v;
}
// the records [R][C] (R <= 4) in order, piece k into ok; a null output is skipped
__global__ void k_fold_ln(const float* __restrict__ part, int64_t S, int R, int C, float* __restrict__ o0, float* __restrict__ o1,
                          float* __restrict__ o2, float* __restrict__ o3) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= R * C) return;
  const int k = e / C;
  float* out = k == 0 ? o0 : k == 1 ? o1 : k == 2 ? o2 : o3;
  if (!out) return;
  float v = part[e];
  for (int64_t s = 1; s < S; s++) v += part[s * R * C + e];
  out[e % C] = v;
}

// ---- host: the rules the plans share --------------------------------------------------------------------------------------
constexpr int kFfnFoldTiles = 64;    // LayerNorm partials: up to this many tiles fold in one level
constexpr int kFfnMaxSlices = 64;    // weight gradients: at most this many row slices, the leaves of k_ffn_fold_params' tree

size_t round256(size_t b) { return (b + 255) / 256 * 256; }
unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

struct Carve {  // a workspace cut into pieces, each at a multiple of 256 bytes
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off += round256(bytes);
    return at;
  }
};
// row slices of a weight gradient of wt 64 x 64 tiles: about 1024 workgroups, a slice no shorter than 64 rows
int weight_slices(int64_t wt, int64_t N) {
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(kFfnMaxSlices, 1024 / wt));
  return (int)std::max<int64_t>(1, std::min<int64_t>(cap, (N + 63) / 64));
}
int64_t slice_rows(int64_t N, int sw) { return ((N + sw - 1) / sw + KC - 1) / KC * KC; }  // rows of a slice, whole KC
// first-level groups of the tiles' partials (0: one level) and the tiles per group
void fold_groups(int64_t tiles, int64_t& groups, int64_t& gper) {
  groups = tiles > kFfnFoldTiles ? std::min<int64_t>(256, (tiles + kFfnFoldTiles - 1) / kFfnFoldTiles) : 0;
  gper = groups ? (tiles + groups - 1) / groups : 0;
}
// f(std::integral_constant<int, NJ>) for the narrowest instantiation that holds C channels
template <typename F>
void with_nj(int C, F f) {
  if (C <= 32) f(std::integral_constant<int, 1>{});
  else if (C <= 64) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}
// dgamma, dbeta of R / 2 LayerNorms from the tiles' records [R][C], in tile order: through `grouped` beyond kFfnFoldTiles tiles
void fold_ln_partials(const float* lnpart, float* grouped, int64_t tiles, int64_t groups, int64_t gper, int R, int C,
                      float* o0, float* o1, float* o2, float* o3, hipStream_t st) {
  const float* rec = lnpart;
  int64_t count = tiles;
  if (groups) {
    k_ffn_fold_groups<<<dim3(blocks_for(R * C, 256), (unsigned)groups), 256, 0, st>>>(lnpart, tiles, R * C, gper, grouped);
    rec = grouped;
    count = groups;
  }
  k_fold_ln<<<blocks_for(R * C, 256), 256, 0, st>>>(rec, count, R, C, o0, o1, o2, o3);
}

}  // namespace
