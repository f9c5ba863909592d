// gcs_sparse.hip -- MI355X (gfx950) kernels + C ABI (include/gcs.h) of the point backbone's sparse operators:
// submanifold 3-D convolution (spconv SubMConv3d) and segment_csr (torch_scatter).  DESIGN.md section 15.
//
// Rulebook (built once per indice_key, reused by every convolution of a stage):
//   * open-addressing hash of packed (b, d0, d1, d2) keys, 64-bit atomicCAS insert, atomicMin picks the
//     lowest row of a voxel as its representative;
//   * neighbour map nbr [N][K] (-1 = absent) and rep [N] (the representative of the row's own voxel);
//   * per tap, the rows that have that neighbour, in row order (pair lists for dW; deterministic scan);
//   * when voxels hold several rows: per representative, its rows in row order (the fold of dy for dX).
// Convolution: output-stationary gather-GEMM on the VALU.  A workgroup owns TM rows x TN output columns; per tap
// it loads the tile's neighbour rows, skips the tap when none is present (block-uniform), and runs an LDS-tiled
// fp32 FMA GEMM of the gathered rows against W[:, k, :].  dX is the same kernel with mirrored taps and W read
// transposed, on dy folded onto the representatives.  dW: per tap, a GEMM over the tap's pair list, cut into a
// fixed number of slices that are summed in slice order.  Every sum has a fixed order: no float atomics.
// Opt-in second engine (GCS_ENGINE_MFMA, gcs_mfma.h): the same three products (forward, dX, dW) on the f32 matrix cores,
// the gather-GEMM in tap slices where the tile grid cannot fill the GPU; the entry points without `_engine` in their
// names are the VALU engine.
// Binary16 (GCS_F16 of the `_t` entry points, gcs_mfma.h): the same products on v_mfma_f32_16x16x16_f16 under the
// matrix-core engine's plan; binary16 segment_csr.  Everything outside the three products is one kernel and one host
// path for both element types T (float, half_t): sums are fp32 in a fixed order, T is converted on the load and ONCE
// on the final store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "../../include/gcs.h"
#define GC_ERR_HIP GCS_ERR_HIP
#include "gc_host.h"

namespace {

typedef _Float16 half_t;  // binary16, the element type of GCS_F16

constexpr uint64_t kEmpty = ~0ull;
constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 16;
constexpr int kScanChunk = kScanThreads * kScanPerThread;  // rows per block of the deterministic scans
constexpr int kMaxK = 1024;                                // taps: up to 9 x 9 x 9 plus headroom

size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

uint64_t table_capacity(int64_t n) {
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n) cap <<= 1;
  return cap;
}

int64_t scan_blocks(int64_t n) { return (n + kScanChunk - 1) / kScanChunk; }

// ---- rulebook layout (device buffer of gcs_subm_rulebook_bytes) ------------------------------------------------
struct Rulebook {
  int32_t* hdr;     // [4 + K]: 0 invalid rows, 1 duplicate flag, 4 + k pairs of tap k
  int32_t* nbr;     // [N][K]
  int32_t* rep;     // [N]
  int32_t* prow;    // [K][N] rows that have tap k, ascending
  int32_t* gstart;  // [N] first entry of a representative's group in glist
  int32_t* gcnt;    // [N] rows of a representative's voxel (0 for the other rows)
  int32_t* glist;   // [N] rows grouped by representative, ascending within a group
  size_t bytes;
};
Rulebook carve_rulebook(void* base, int64_t n, int32_t k) {
  Rulebook r;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t b) {
    char* q = p ? p + off : nullptr;
    off += align_up(b);
    return (int32_t*)q;
  };
  r.hdr = take(4 * (4 + (size_t)k));
  r.nbr = take(4 * (size_t)n * k);
  r.rep = take(4 * (size_t)n);
  r.prow = take(4 * (size_t)n * k);
  r.gstart = take(4 * (size_t)n);
  r.gcnt = take(4 * (size_t)n);
  r.glist = take(4 * (size_t)n);
  r.bytes = off;
  return r;
}
struct Scratch {
  uint64_t* keys;   // [cap]
  int32_t* vals;    // [cap] representative row of the slot
  int32_t* gfill;   // [N]
  int32_t* bsum;    // [K][blocks] scan block totals
  size_t bytes;
};
Scratch carve_scratch(void* base, int64_t n) {
  Scratch s;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t b) {
    char* q = p ? p + off : nullptr;
    off += align_up(b);
    return q;
  };
  const uint64_t cap = table_capacity(n);
  s.keys = (uint64_t*)take(8 * cap);
  s.vals = (int32_t*)take(4 * cap);
  s.gfill = (int32_t*)take(4 * (size_t)n);
  s.bsum = (int32_t*)take(4 * (size_t)kMaxK * scan_blocks(n));
  s.bytes = off;
  return s;
}

// ---- hash table --------------------------------------------------------------------------------------------------
struct Geom {
  int32_t batch, s0, s1, s2;
  int32_t k0, k1, k2, dl0, dl1, dl2;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ bool row_valid(const int32_t* idx, int64_t i, const Geom& g) {
  const int b = idx[4 * i], a = idx[4 * i + 1], c = idx[4 * i + 2], d = idx[4 * i + 3];
  return b >= 0 && b < g.batch && a >= 0 && a < g.s0 && c >= 0 && c < g.s1 && d >= 0 && d < g.s2;
}
__device__ __forceinline__ uint64_t pack(int b, int a, int c, int d, const Geom& g) {
  return (((uint64_t)b * (uint64_t)g.s0 + (uint64_t)a) * (uint64_t)g.s1 + (uint64_t)c) * (uint64_t)g.s2 + (uint64_t)d;
}
__device__ __forceinline__ int32_t lookup(const uint64_t* keys, const int32_t* vals, uint64_t mask, uint64_t key) {
  uint64_t slot = mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    const uint64_t k = keys[slot];
    if (k == key) return vals[slot];
    if (k == kEmpty) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

__global__ void k_insert(const int32_t* __restrict__ idx, int64_t n, Geom g, uint64_t* keys, int32_t* vals,
                         uint64_t mask, int32_t* hdr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!row_valid(idx, i, g)) {
    atomicAdd(&hdr[0], 1);
    return;
  }
  const uint64_t key = pack(idx[4 * i], idx[4 * i + 1], idx[4 * i + 2], idx[4 * i + 3], g);
  uint64_t slot = mix64(key) & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    const unsigned long long prev =
        atomicCAS((unsigned long long*)&keys[slot], (unsigned long long)kEmpty, (unsigned long long)key);
    if (prev == kEmpty || prev == key) {
      atomicMin(&vals[slot], (int32_t)i);
      return;
    }
    slot = (slot + 1) & mask;
  }
}

// one thread per (row, tap); the centre tap also records the row's representative and the duplicate flag
__global__ void k_neighbours(const int32_t* __restrict__ idx, int64_t n, Geom g, const uint64_t* __restrict__ keys,
                             const int32_t* __restrict__ vals, uint64_t mask, int32_t* __restrict__ nbr,
                             int32_t* __restrict__ rep, int32_t* hdr) {
  const int K = g.k0 * g.k1 * g.k2;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * K) return;
  const int64_t i = e / K;
  const int k = (int)(e - i * K);
  int32_t j = -1;
  if (row_valid(idx, i, g)) {
    const int ta = k / (g.k1 * g.k2), tb = (k / g.k2) % g.k1, tc = k % g.k2;
    const int a = idx[4 * i + 1] + (ta - g.k0 / 2) * g.dl0;
    const int b = idx[4 * i + 2] + (tb - g.k1 / 2) * g.dl1;
    const int c = idx[4 * i + 3] + (tc - g.k2 / 2) * g.dl2;
    if (a >= 0 && a < g.s0 && b >= 0 && b < g.s1 && c >= 0 && c < g.s2)
      j = lookup(keys, vals, mask, pack(idx[4 * i], a, b, c, g));
  }
  nbr[e] = j;
  if (k == K / 2) {
    rep[i] = j;
    if (j >= 0 && j != (int32_t)i) atomicOr(&hdr[1], 1);
  }
}

// ---- deterministic block scans (pair lists per tap, duplicate groups) --------------------------------------------
// MODE 0: value of row i in column k (= blockIdx.y) is nbr[i][k] >= 0; pass 3 writes prow[k][offset] = i.
// MODE 1: value of row i is gcnt[i] (only when hdr[1], the duplicate flag, is set); pass 3 writes gstart[i].
template <int MODE>
__device__ __forceinline__ int scan_value(const int32_t* src, int64_t i, int k, int K) {
  return MODE == 0 ? (src[i * K + k] >= 0 ? 1 : 0) : src[i];
}

__device__ int block_exclusive_scan(int v, int* sh, int* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {
    const int add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int incl = sh[t];
  *total = sh[kScanThreads - 1];
  __syncthreads();
  return incl - v;
}

template <int MODE>
__global__ __launch_bounds__(kScanThreads) void k_scan_count(const int32_t* __restrict__ src, int64_t n, int K,
                                                             const int32_t* hdr, int32_t* __restrict__ bsum) {
  if (MODE == 1 && hdr[1] == 0) return;
  __shared__ int sh[kScanThreads];
  const int k = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPerThread;
  int v = 0;
  for (int q = 0; q < kScanPerThread; q++)
    if (r0 + q < n) v += scan_value<MODE>(src, r0 + q, k, K);
  int total;
  block_exclusive_scan(v, sh, &total);
  if (threadIdx.x == 0) bsum[(int64_t)k * gridDim.x + blockIdx.x] = total;
}

// one thread per column: block totals -> exclusive block offsets (in place), column total into hdr[4 + k]
template <int MODE>
__global__ void k_scan_blocks(int32_t* bsum, int64_t nb, int K, int32_t* hdr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K || (MODE == 1 && hdr[1] == 0)) return;
  int run = 0;
  for (int64_t b = 0; b < nb; b++) {
    const int v = bsum[(int64_t)k * nb + b];
    bsum[(int64_t)k * nb + b] = run;
    run += v;
  }
  if (MODE == 0) hdr[4 + k] = run;
}

template <int MODE>
__global__ __launch_bounds__(kScanThreads) void k_scan_write(const int32_t* __restrict__ src, int64_t n, int K,
                                                             const int32_t* hdr, const int32_t* __restrict__ bsum,
                                                             int32_t* __restrict__ dst) {
  if (MODE == 1 && hdr[1] == 0) return;
  __shared__ int sh[kScanThreads];
  const int k = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPerThread;
  int v = 0;
  for (int q = 0; q < kScanPerThread; q++)
    if (r0 + q < n) v += scan_value<MODE>(src, r0 + q, k, K);
  int total;
  int off = block_exclusive_scan(v, sh, &total) + bsum[(int64_t)k * gridDim.x + blockIdx.x];
  for (int q = 0; q < kScanPerThread; q++) {
    const int64_t i = r0 + q;
    if (i >= n) break;
    const int x = scan_value<MODE>(src, i, k, K);
    if (MODE == 0) {
      if (x) dst[(int64_t)k * n + off] = (int32_t)i;
    } else {
      dst[i] = off;
    }
    off += x;
  }
}

__global__ void k_group_count(const int32_t* __restrict__ rep, int64_t n, const int32_t* hdr, int32_t* gcnt) {
  if (hdr[1] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && rep[i] >= 0) atomicAdd(&gcnt[rep[i]], 1);
}
__global__ void k_group_fill(const int32_t* __restrict__ rep, int64_t n, const int32_t* hdr,
                             const int32_t* __restrict__ gstart, int32_t* gfill, int32_t* glist) {
  if (hdr[1] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || rep[i] < 0) return;
  const int r = rep[i];
  glist[gstart[r] + atomicAdd(&gfill[r], 1)] = (int32_t)i;
}
// groups are small (rows of one voxel): insertion sort puts each in row order, the representative first
__global__ void k_group_sort(int64_t n, const int32_t* hdr, const int32_t* __restrict__ gstart,
                             const int32_t* __restrict__ gcnt, int32_t* glist) {
  if (hdr[1] == 0) return;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || gcnt[r] < 2) return;
  int32_t* g = glist + gstart[r];
  for (int a = 1; a < gcnt[r]; a++) {
    const int32_t v = g[a];
    int b = a - 1;
    for (; b >= 0 && g[b] > v; b--) g[b + 1] = g[b];
    g[b + 1] = v;
  }
}

// ---- convolution ---------------------------------------------------------------------------------------------
// y[row][o] = bias[o] + sum_k sum_c W(k, o, c) * x[nbr[row][tap(k)]][c],  W(k, o, c) = w[k*sk + o*sn + c*sc],
// tap(k) = k, or K-1-k (mirror, for dX).  rowmask: rows with rowmask[row] != row are written 0 (dX of duplicates).
// 256 threads; a thread owns MR rows x MC columns; TRANS picks the coalesced order of the weight tile load.
constexpr int KC = 16;
constexpr int KR = 16;  // pairs per LDS chunk of the dW kernels (k_subm_dw below, k_subm_dw_mfma in gcs_mfma.h)

// The head of a tap, shared by the gather-GEMM kernels of both engines and both element types: the tile's neighbour
// rows under tap k of the loop order go to sN (-1 = absent, and beyond n); returns whether any row of the tile has the
// tap.  The answer is block-uniform (__syncthreads_or), so a workgroup skips an absent tap as one.
template <int TM>
__device__ __forceinline__ int tap_head(const int32_t* __restrict__ nbr, int K, int k, int mirror, int64_t row0, int64_t n,
                                        int32_t* sN) {
  const int kn = mirror ? K - 1 - k : k;
  int any = 0;
  for (int r = threadIdx.x; r < TM; r += 256) {
    const int64_t row = row0 + r;
    const int32_t j = row < n ? nbr[row * K + kn] : -1;
    sN[r] = j;
    any |= j >= 0;
  }
  return __syncthreads_or(any);
}
// The one store of an output element whose fp32 sum is s: into the fp32 partials when the sum continues elsewhere
// (`part`), else the final value -- 0 for a row the mask excludes, the bias added in fp32, ONE conversion to T.
template <typename T>
__device__ __forceinline__ void store_out(float s, int64_t at, int o, bool zero, const T* bias, T* y, float* part) {
  if (part)
    part[at] = s;
  else
    y[at] = (T)(zero ? 0.0f : (bias ? s + (float)bias[o] : s));
}
template <int TM, int TN, int MR, int MC, bool TRANS>
__global__ __launch_bounds__(256) void k_subm_gemm(const float* __restrict__ x, int cin, const float* __restrict__ w,
                                                   int64_t sk, int64_t sn, int64_t sc, const float* __restrict__ bias,
                                                   const int32_t* __restrict__ nbr, int K, int mirror,
                                                   const int32_t* __restrict__ rowmask, float* __restrict__ y, int nout,
                                                   int64_t n) {
  constexpr int TCX = TN / MC, TCY = 256 / TCX;
  static_assert(TCY * MR == TM, "tile shape");
  __shared__ float As[KC][TM];
  __shared__ float Bs[KC][TN];
  __shared__ int32_t sN[TM];
  const int tid = threadIdx.x, tx = tid % TCX, ty = tid / TCX;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n0 = blockIdx.y * TN;
  float acc[MR][MC];
#pragma unroll
  for (int i = 0; i < MR; i++)
#pragma unroll
    for (int j = 0; j < MC; j++) acc[i][j] = 0.0f;

  for (int k = 0; k < K; k++) {
    if (!tap_head<TM>(nbr, K, k, mirror, row0, n, sN)) continue;
    for (int c0 = 0; c0 < cin; c0 += KC) {
      for (int e = tid; e < TM * KC; e += 256) {
        const int r = e / KC, cc = e % KC, c = c0 + cc;
        const int32_t j = sN[r];
        As[cc][r] = (j >= 0 && c < cin) ? x[(int64_t)j * cin + c] : 0.0f;
      }
      for (int e = tid; e < TN * KC; e += 256) {
        const int cc = TRANS ? e / TN : e % KC, nn = TRANS ? e % TN : e / KC;
        const int c = c0 + cc, o = n0 + nn;
        Bs[cc][nn] = (c < cin && o < nout) ? w[(int64_t)k * sk + (int64_t)o * sn + (int64_t)c * sc] : 0.0f;
      }
      __syncthreads();
#pragma unroll
      for (int cc = 0; cc < KC; cc++) {
        float a[MR], b[MC];
#pragma unroll
        for (int i = 0; i < MR; i++) a[i] = As[cc][ty * MR + i];
#pragma unroll
        for (int j = 0; j < MC; j++) b[j] = Bs[cc][tx * MC + j];
#pragma unroll
        for (int i = 0; i < MR; i++)
#pragma unroll
          for (int j = 0; j < MC; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int i = 0; i < MR; i++) {
    const int64_t row = row0 + ty * MR + i;
    if (row >= n) continue;
    const bool zero = rowmask && rowmask[row] != (int32_t)row;
#pragma unroll
    for (int j = 0; j < MC; j++) {
      const int o = n0 + tx * MC + j;
      if (o < nout) y[row * nout + o] = zero ? 0.0f : (bias ? acc[i][j] + bias[o] : acc[i][j]);  // store_out, final
    }
  }
}

// ---- the launches of the gather-GEMM and of dW: one argument block, one tile dispatch each --------------------------
// y[n][nout] = bias + sum over the taps of x[nbr[.][tap]] . W(k), in the terms of k_subm_gemm above
template <typename T>
struct Gemm {
  const T* x;
  int cin;
  const T* w;
  int64_t sk, sn, sc;
  const T* bias;
  const int32_t* nbr;
  int K, mirror;
  const int32_t* rowmask;
  T* y;
  int nout;
  int64_t n;
};
template <int TM_, int TN_>
struct Tile {
  static constexpr int TM = TM_, TN = TN_;
};
unsigned blocks_for(int64_t items, int threads) { return (unsigned)((items + threads - 1) / threads); }

// GCS_TILE_* of a gather-GEMM -> launch(Tile<TM, TN>, grid): TM x TN tiles over n x nout, S tap slices
template <typename F>
void for_gemm_tile(int tile, int64_t n, int nout, int S, F&& launch) {
  if (tile == GCS_TILE_64X64)
    launch(Tile<64, 64>(), dim3(blocks_for(n, 64), blocks_for(nout, 64), (unsigned)S));
  else if (tile == GCS_TILE_128X32)
    launch(Tile<128, 32>(), dim3(blocks_for(n, 128), 1, (unsigned)S));  // nout <= 32: one column tile
  else
    launch(Tile<32, 32>(), dim3(blocks_for(n, 32), blocks_for(nout, 32), (unsigned)S));
}
// GCS_TILE_* of dW -> launch(Tile<T, T>, grid): T x T tiles over cout x cin, per tap, S pair slices
template <typename F>
void for_dw_tile(int tile, int cin, int cout, int K, int S, F&& launch) {
  if (tile == GCS_TILE_64X64)
    launch(Tile<64, 64>(), dim3(blocks_for(cout, 64) * blocks_for(cin, 64), (unsigned)K, (unsigned)S));
  else
    launch(Tile<32, 32>(), dim3(blocks_for(cout, 32) * blocks_for(cin, 32), (unsigned)K, (unsigned)S));
}

template <bool TRANS>
void launch_gemm(int tile, const Gemm<float>& g, hipStream_t st) {
  for_gemm_tile(tile, g.n, g.nout, 1, [&](auto t, dim3 grid) {
    constexpr int TM = decltype(t)::TM, TN = decltype(t)::TN, M = TM * TN == 32 * 32 ? 2 : 4;  // M x M per thread
    k_subm_gemm<TM, TN, M, M, TRANS><<<grid, 256, 0, st>>>(g.x, g.cin, g.w, g.sk, g.sn, g.sc, g.bias, g.nbr, g.K, g.mirror,
                                                           g.rowmask, g.y, g.nout, g.n);
  });
}

#include "gcs_mfma.h"

// dw partial of slice s: part[s][o][k][c] = sum over the slice's pairs p of tap k: dy[i_p][o] * x[nbr[i_p][k]][c]
template <int TO, int TC, int MR, int MC>
__global__ __launch_bounds__(256) void k_subm_dw(const float* __restrict__ dy, int cout, const float* __restrict__ x,
                                                 int cin, const int32_t* __restrict__ nbr, int K,
                                                 const int32_t* __restrict__ prow, const int32_t* __restrict__ hdr,
                                                 int64_t n, int nslice, float* __restrict__ part) {
  constexpr int TCX = TC / MC, TCY = 256 / TCX;
  static_assert(TCY * MR == TO, "tile shape");
  __shared__ float Ds[KR][TO];
  __shared__ float Xs[KR][TC];
  __shared__ int32_t sI[KR], sJ[KR];
  const int tid = threadIdx.x, tx = tid % TCX, ty = tid / TCX;
  const int tiles_c = (cin + TC - 1) / TC;
  const int o0 = (blockIdx.x / tiles_c) * TO, c0 = (blockIdx.x % tiles_c) * TC;
  const int k = blockIdx.y, s = blockIdx.z;
  const int64_t cnt = hdr[4 + k];
  const int64_t per = (cnt + nslice - 1) / nslice;
  const int64_t p0 = s * per, p1 = p0 + per < cnt ? p0 + per : cnt;
  float acc[MR][MC];
#pragma unroll
  for (int i = 0; i < MR; i++)
#pragma unroll
    for (int j = 0; j < MC; j++) acc[i][j] = 0.0f;
  for (int64_t p = p0; p < p1; p += KR) {
    if (tid < KR) {
      const int64_t q = p + tid;
      const int32_t i = q < p1 ? prow[(int64_t)k * n + q] : -1;
      sI[tid] = i;
      sJ[tid] = i >= 0 ? nbr[(int64_t)i * K + k] : -1;
    }
    __syncthreads();
    for (int e = tid; e < KR * TO; e += 256) {
      const int r = e / TO, o = o0 + e % TO;
      const int32_t i = sI[r];
      Ds[r][e % TO] = (i >= 0 && o < cout) ? dy[(int64_t)i * cout + o] : 0.0f;
    }
    for (int e = tid; e < KR * TC; e += 256) {
      const int r = e / TC, c = c0 + e % TC;
      const int32_t j = sJ[r];
      Xs[r][e % TC] = (j >= 0 && c < cin) ? x[(int64_t)j * cin + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KR; r++) {
      float a[MR], b[MC];
#pragma unroll
      for (int i = 0; i < MR; i++) a[i] = Ds[r][ty * MR + i];
#pragma unroll
      for (int j = 0; j < MC; j++) b[j] = Xs[r][tx * MC + j];
#pragma unroll
      for (int i = 0; i < MR; i++)
#pragma unroll
        for (int j = 0; j < MC; j++) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* out = part + (int64_t)s * cout * K * cin;
#pragma unroll
  for (int i = 0; i < MR; i++) {
    const int o = o0 + ty * MR + i;
    if (o >= cout) continue;
#pragma unroll
    for (int j = 0; j < MC; j++) {
      const int c = c0 + tx * MC + j;
      if (c < cin) out[((int64_t)o * K + k) * cin + c] = acc[i][j];
    }
  }
}

// the VALU launch of dW; `part` is [S][cout][K][cin] when S > 1, else dw itself receives the sums
void launch_dw(int tile, int S, const float* dy, int cout, const float* x, int cin, const int32_t* nbr, int K,
               const int32_t* prow, const int32_t* hdr, int64_t n, float* part, float* dw, hipStream_t st) {
  for_dw_tile(tile, cin, cout, K, S, [&](auto t, dim3 grid) {
    constexpr int T = decltype(t)::TM;
    k_subm_dw<T, T, T / 16, T / 16><<<grid, 256, 0, st>>>(dy, cout, x, cin, nbr, K, prow, hdr, n, S, S > 1 ? part : dw);
  });
}

// ---- the element-wise kernels, one for both element types T: fp32 sums in a fixed order, T converted on the load and
// once on the store (no conversion at all for float) ------------------------------------------------------------------
// out[e] = T(sum_s part[s][e]), s ascending
template <typename T>
__global__ void k_sum_slices(const float* __restrict__ part, int nslice, int64_t len, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  float v = part[e];
  for (int s = 1; s < nslice; s++) v += part[(int64_t)s * len + e];
  out[e] = (T)v;
}

// column sums of dy over a slice of rows: 64 columns x 4 row phases per block, phases combined in order
template <typename T>
__global__ __launch_bounds__(256) void k_colsum(const T* __restrict__ dy, int64_t n, int cout, int nslice,
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

// dyf[r] = T(fp32 sum of dy over the rows of representative r's voxel, row order); other rows are never read
template <typename T>
__global__ void k_fold(const T* __restrict__ dy, int64_t n, int cout, const int32_t* __restrict__ rep,
                       const int32_t* __restrict__ gstart, const int32_t* __restrict__ gcnt,
                       const int32_t* __restrict__ glist, T* __restrict__ dyf) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * cout) return;
  const int64_t r = e / cout;
  const int o = (int)(e - r * cout);
  if (rep[r] != (int32_t)r) return;
  const int cnt = gcnt[r];
  if (cnt < 2) {  // a voxel of one row (or groups never built: the rulebook had no duplicates)
    dyf[e] = dy[e];
    return;
  }
  const int32_t* g = glist + gstart[r];
  float v = (float)dy[(int64_t)g[0] * cout + o];
  for (int q = 1; q < cnt; q++) v += (float)dy[(int64_t)g[q] * cout + o];
  dyf[e] = (T)v;
}

// ---- segment_csr -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void seg_bounds(const int64_t* indptr, int64_t s, int64_t m, int64_t* lo, int64_t* hi) {
  int64_t a = indptr[s], b = indptr[s + 1];
  a = a < 0 ? 0 : (a > m ? m : a);
  b = b < a ? a : (b > m ? m : b);
  *lo = a;
  *hi = b;
}

// one wave per (segment, block of 64 columns).  Sum and mean: fp32 in row order, mean divided in fp32, one conversion
// to T.  Min and max compare exactly and copy bits; the arg is the first row that attains the value.
template <typename T>
__global__ __launch_bounds__(64) void k_seg_fwd(const T* __restrict__ src, int64_t m, int64_t f,
                                                const int64_t* __restrict__ indptr, int64_t nfb, int reduce,
                                                T* __restrict__ out, int64_t* __restrict__ arg) {
  const int64_t s = blockIdx.x / nfb, col = (blockIdx.x % nfb) * 64 + threadIdx.x;
  if (col >= f) return;
  int64_t lo, hi;
  seg_bounds(indptr, s, m, &lo, &hi);
  T res = (T)0.0f;
  int64_t best = -1;
  if (reduce == GCS_SUM || reduce == GCS_MEAN) {
    float v = 0.0f;
    for (int64_t r = lo; r < hi; r++) v += (float)src[r * f + col];
    if (reduce == GCS_MEAN && hi > lo) v = v / (float)(hi - lo);
    res = (T)v;
  } else if (hi > lo) {
    res = src[lo * f + col];
    best = lo;
    for (int64_t r = lo + 1; r < hi; r++) {
      const T u = src[r * f + col];
      if (reduce == GCS_MAX ? (float)u > (float)res : (float)u < (float)res) {
        res = u;
        best = r;
      }
    }
  }
  out[s * f + col] = res;
  if (arg) arg[s * f + col] = best;
}

template <typename T>
__global__ __launch_bounds__(64) void k_seg_bwd(const T* __restrict__ dout, int64_t m, int64_t f,
                                                const int64_t* __restrict__ indptr, int64_t nfb, int reduce,
                                                const int64_t* __restrict__ arg, T* __restrict__ dsrc) {
  const int64_t s = blockIdx.x / nfb, col = (blockIdx.x % nfb) * 64 + threadIdx.x;
  if (col >= f) return;
  int64_t lo, hi;
  seg_bounds(indptr, s, m, &lo, &hi);
  T g = dout[s * f + col];
  if (reduce == GCS_MEAN && hi > lo) g = (T)((float)g / (float)(hi - lo));
  const int64_t a = (reduce == GCS_MIN || reduce == GCS_MAX) ? arg[s * f + col] : -1;
  for (int64_t r = lo; r < hi; r++)
    dsrc[r * f + col] = (reduce == GCS_SUM || reduce == GCS_MEAN) ? g : (r == a ? g : (T)0.0f);
}

// ---- host helpers ----------------------------------------------------------------------------------------------
int check_conv_dims(const char* who, int64_t n, int32_t K, int32_t cin, int32_t cout) {
  if (n < 0 || n > (int64_t)INT32_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": n out of range");
  if (K < 1 || K > kMaxK || n * (int64_t)K > (int64_t)INT32_MAX)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": kernel volume out of range");
  if (cin < 1 || cout < 1 || cin > 65536 || cout > 65536)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": channel count out of range");
  return 0;
}

// ---- the plan: every shape-dependent choice of the convolution, made here and nowhere else ---------------------
// Tile of k_subm_gemm for n rows x nout output columns: 64 x 64 or 128 x 32 (4 x 4 per thread) once they give the
// GPU 256 workgroups, 32 x 32 (2 x 2 per thread) for the small grids below that.
int gemm_tile(int64_t n, int32_t nout) {
  const int64_t wide = ((n + 63) / 64) * ((nout + 63) / 64), tall = (n + 127) / 128;
  if (nout > 32 && wide >= 256) return GCS_TILE_64X64;
  if (nout > 16 && nout <= 32 && tall >= 256) return GCS_TILE_128X32;
  return GCS_TILE_32X32;
}
// slices of the dW reduction: enough workgroups to fill the GPU, a function of the shape only
int dw_slices(int64_t n, int32_t cin, int32_t cout, int32_t K, int tile) {
  const int t = tile == GCS_TILE_64X64 ? 64 : 32;
  const int64_t wgs = (int64_t)((cout + t - 1) / t) * ((cin + t - 1) / t) * K;
  int64_t s = (2048 + wgs - 1) / wgs;
  const int64_t by_rows = n / 256 > 1 ? n / 256 : 1;  // at least ~256 rows per slice
  s = s < by_rows ? s : by_rows;
  return (int)(s < 1 ? 1 : (s > 32 ? 32 : s));
}
int colsum_slices(int64_t n) {
  const int64_t s = n / 2048;
  return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}
struct Plan {
  int32_t fwd, dx, dw, dw_slices, db_slices;  // the order of gcs_subm_plan's output
};
Plan plan_of(int64_t n, int32_t cin, int32_t cout, int32_t K) {
  Plan p;
  p.fwd = gemm_tile(n, cout);
  p.dx = gemm_tile(n, cin);
  p.dw = (cin >= 64 && cout >= 64) ? GCS_TILE_64X64 : GCS_TILE_32X32;
  p.dw_slices = dw_slices(n, cin, cout, K, p.dw);
  p.db_slices = colsum_slices(n);
  return p;
}

// Tap slices of the matrix-core engine for an n x nout gemm over K taps under `tile`: 1 once the tile grid has 256
// workgroups (a shape that fills the GPU keeps the VALU engine's values), below that enough slices for about
// GCS_SLICE_TARGET workgroups, normalised so that no slice is empty.  A function of (n, nout, K) only.
#ifndef GCS_SLICE_TARGET
#define GCS_SLICE_TARGET 512
#endif
int tap_slices(int64_t n, int32_t nout, int32_t K, int tile) {
  const int tm = tile == GCS_TILE_64X64 ? 64 : tile == GCS_TILE_128X32 ? 128 : 32;
  const int tn = tile == GCS_TILE_64X64 ? 64 : 32;
  const int64_t wgs = ((n + tm - 1) / tm) * ((nout + tn - 1) / tn);
  if (wgs == 0 || wgs >= 256) return 1;
  int64_t s = ((int64_t)GCS_SLICE_TARGET + wgs - 1) / wgs;
  s = s < 1 ? 1 : (s > K ? K : s);
  const int64_t per = (K + s - 1) / s;
  return (int)((K + per - 1) / per);
}
struct EnginePlan {
  Plan p;
  int32_t fwd_slices, dx_slices;  // tap slices of the forward and of dX: 1, 1 for the VALU engine
};
EnginePlan engine_plan_of(int32_t engine, int64_t n, int32_t cin, int32_t cout, int32_t K) {
  EnginePlan e;
  e.p = plan_of(n, cin, cout, K);
  const bool mfma = engine == GCS_ENGINE_MFMA;
  e.fwd_slices = mfma ? tap_slices(n, cout, K, e.p.fwd) : 1;
  e.dx_slices = mfma ? tap_slices(n, cin, K, e.p.dx) : 1;
  return e;
}
int check_engine(const char* who, int32_t engine) {
  if (engine != GCS_ENGINE_VALU && engine != GCS_ENGINE_MFMA)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown engine (GCS_ENGINE_VALU or GCS_ENGINE_MFMA)");
  return 0;
}
size_t forward_ws_bytes(const EnginePlan& e, int64_t n, int32_t cout) {
  return e.fwd_slices > 1 ? align_up(4 * (size_t)e.fwd_slices * n * cout) : 0;
}

// ---- the host path of the convolution, one for both element types T ------------------------------------------------
int check_dtype(const char* who, int32_t dtype) {
  if (dtype != GCS_F32 && dtype != GCS_F16)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown dtype (GCS_F32 or GCS_F16)");
  return 0;
}
// binary16 pointers are 2-byte aligned (float pointers are taken as they come)
template <typename T>
int check_pointers(const char* who, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (sizeof(T) == 2 && ((uintptr_t)p & 1))
      return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": a binary16 pointer is not 2-byte aligned");
  return 0;
}
// a workspace of a binary16 call holds fp32 partials
template <typename T>
int check_workspace_alignment(const char* who, const void* workspace) {
  if (sizeof(T) == 2 && ((uintptr_t)workspace & 3))
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": the workspace is not 4-byte aligned");
  return 0;
}

// What an entry point runs: the engine (binary16 has one, the matrix cores under engine_plan_of(GCS_ENGINE_MFMA)) and
// the workspace query its error text cites.
struct Route {
  int32_t engine;
  const char* ws_query;
};
Route route_f32(int32_t engine) {
  return Route{engine, engine == GCS_ENGINE_VALU ? "gcs_subm_backward_workspace_bytes" : "gcs_subm_engine_workspace_bytes"};
}
const Route kRouteF16{GCS_ENGINE_MFMA, "gcs_subm_workspace_bytes_t"};

template <typename T>
struct BwdWs {
  T* dyf;       // [N][Cout] when dups: the fold, in the element type
  float* dwp;   // [S][Cout][K][Cin] when S > 1
  float* dbp;   // [Sb][Cout]
  float* dxp;   // [Sx][N][Cin] when dX runs in Sx > 1 tap slices (matrix cores)
  size_t bytes;
};
template <typename T>
BwdWs<T> carve_bwd(void* base, const EnginePlan& e, int64_t n, int32_t cin, int32_t cout, int32_t K, int32_t dups) {
  BwdWs<T> w;
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t b) {
    char* q = (p && b) ? p + off : nullptr;
    off += align_up(b);
    return (void*)q;
  };
  w.dyf = (T*)take(dups ? sizeof(T) * (size_t)n * cout : 0);
  w.dwp = (float*)take(e.p.dw_slices > 1 ? 4 * (size_t)e.p.dw_slices * cout * K * cin : 0);
  w.dbp = (float*)take(4 * (size_t)e.p.db_slices * cout);
  w.dxp = (float*)take(e.dx_slices > 1 ? 4 * (size_t)e.dx_slices * n * cin : 0);
  w.bytes = off;
  return w;
}

// the gather-GEMM and dW of a route: the VALU kernels exist for float only
template <bool TRANS, typename T>
void run_gemm(int32_t engine, int tile, int S, const Gemm<T>& g, float* part, hipStream_t st) {
  if constexpr (std::is_same<T, float>::value)
    if (engine == GCS_ENGINE_VALU) return launch_gemm<TRANS>(tile, g, st);
  launch_gemm_mfma<TRANS>(tile, S, g, part, st);
}
template <typename T>
void run_dw(int32_t engine, int tile, int S, const T* dy, int cout, const T* x, int cin, const Rulebook& rb, int K, int64_t n,
            float* part, T* dw, hipStream_t st) {
  if constexpr (std::is_same<T, float>::value)
    if (engine == GCS_ENGINE_VALU) return launch_dw(tile, S, dy, cout, x, cin, rb.nbr, K, rb.prow, rb.hdr, n, part, dw, st);
  launch_dw_mfma(tile, S, dy, cout, x, cin, rb.nbr, K, rb.prow, rb.hdr, n, part, dw, st);
}

// the forward and the backward of every route; `who` names the entry point in the error texts
template <typename T>
int subm_forward(const char* who, Route rt, const void* rulebook, int64_t n, int32_t kvol, const T* features, int32_t cin,
                 const T* weight, const T* bias, int32_t cout, T* out, void* workspace, size_t workspace_bytes,
                 void* hip_stream) {
  const std::string me(who);
  if (int rc = check_conv_dims(who, n, kvol, cin, cout)) return rc;
  if (int rc = check_pointers<T>(who, {features, weight, bias, out})) return rc;
  if (!rulebook || !weight) return fail(GCS_ERR_INVALID_ARGUMENT, me + ": null rulebook or weight");
  if (n == 0) return 0;
  if (!features || !out) return fail(GCS_ERR_INVALID_ARGUMENT, me + ": null features or output");
  const EnginePlan e = engine_plan_of(rt.engine, n, cin, cout, kvol);
  const size_t need = forward_ws_bytes(e, n, cout);
  if (need && (!workspace || workspace_bytes < need))
    return fail(GCS_ERR_INVALID_ARGUMENT, me + ": workspace missing or smaller than " + rt.ws_query);
  if (need)
    if (int rc = check_workspace_alignment<T>(who, workspace)) return rc;
  const Rulebook rb = carve_rulebook((void*)rulebook, n, kvol);
  const Gemm<T> g{features, cin, weight, cin, (int64_t)kvol * cin, 1, bias, rb.nbr, kvol, 0, nullptr, out, cout, n};
  run_gemm<false>(rt.engine, e.p.fwd, e.fwd_slices, g, (float*)workspace, (hipStream_t)hip_stream);
  HIP_TRY(hipGetLastError(), "forward launch");
  return 0;
}

template <typename T>
int subm_backward(const char* who, Route rt, const void* rulebook, int64_t n, int32_t kvol, int32_t dups, const T* features,
                  int32_t cin, const T* weight, int32_t cout, const T* dout, T* dx, T* dw, T* db, void* workspace,
                  size_t workspace_bytes, void* hip_stream) {
  const std::string me(who);
  if (int rc = check_conv_dims(who, n, kvol, cin, cout)) return rc;
  if (int rc = check_pointers<T>(who, {features, weight, dout, dx, dw, db})) return rc;
  if (!rulebook || !weight) return fail(GCS_ERR_INVALID_ARGUMENT, me + ": null rulebook or weight");
  const EnginePlan e = engine_plan_of(rt.engine, n, cin, cout, kvol);
  const Plan& pl = e.p;
  const BwdWs<T> ws = carve_bwd<T>(workspace, e, n, cin, cout, kvol, dups);
  if (!workspace || workspace_bytes < ws.bytes)
    return fail(GCS_ERR_INVALID_ARGUMENT, me + ": workspace missing or smaller than " + rt.ws_query);
  if (int rc = check_workspace_alignment<T>(who, workspace)) return rc;
  if (n > 0 && (!dout || ((dx || dw) && !features)))
    return fail(GCS_ERR_INVALID_ARGUMENT, me + ": null features or output gradient");
  hipStream_t st = (hipStream_t)hip_stream;
  const Rulebook rb = carve_rulebook((void*)rulebook, n, kvol);
  if (n == 0) {
    if (dw) HIP_TRY(hipMemsetAsync(dw, 0, sizeof(T) * (size_t)cout * kvol * cin, st), "dw clear");
    if (db) HIP_TRY(hipMemsetAsync(db, 0, sizeof(T) * (size_t)cout, st), "db clear");
    return 0;
  }
  if (dx) {
    const T* gy = dout;
    if (dups) {
      k_fold<T><<<blocks_for(n * cout, 256), 256, 0, st>>>(dout, n, cout, rb.rep, rb.gstart, rb.gcnt, rb.glist, ws.dyf);
      gy = ws.dyf;
    }
    // dX[j][c] = sum_k sum_o W[o][k][c] * gy[nbr[j][K-1-k]][o]: reduction over o (stride K*Cin), output c (stride 1)
    const Gemm<T> g{gy, cout, weight, cin, 1, (int64_t)kvol * cin, nullptr, rb.nbr, kvol, 1, dups ? rb.rep : nullptr,
                    dx, cin, n};
    run_gemm<true>(rt.engine, pl.dx, e.dx_slices, g, ws.dxp, st);
  }
  if (dw) {
    const int S = pl.dw_slices;
    run_dw(rt.engine, pl.dw, S, dout, cout, features, cin, rb, kvol, n, ws.dwp, dw, st);
    if (S > 1) {
      const int64_t len = (int64_t)cout * kvol * cin;
      k_sum_slices<T><<<blocks_for(len, 256), 256, 0, st>>>(ws.dwp, S, len, dw);
    }
  }
  if (db) {
    const int S = pl.db_slices;
    k_colsum<T><<<dim3(blocks_for(cout, 64), (unsigned)S), 256, 0, st>>>(dout, n, cout, S, ws.dbp);
    k_sum_slices<T><<<blocks_for(cout, 256), 256, 0, st>>>(ws.dbp, S, cout, db);
  }
  HIP_TRY(hipGetLastError(), "backward launch");
  return 0;
}

// ---- segment_csr: one typed body per direction ------------------------------------------------------------------
int check_segment(const char* who, const void* a, const void* b, const int64_t* indptr, int64_t m, int64_t f, int64_t s,
                  int32_t reduce, const int64_t* arg, bool arg_read) {
  if (m < 0 || f < 1 || s < 0 || f > (int64_t)INT32_MAX)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": sizes out of range");
  if (reduce < GCS_SUM || reduce > GCS_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown reduce");
  const bool needs_arg = reduce == GCS_MIN || reduce == GCS_MAX;
  if (s > 0 && (!b || !indptr)) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (m > 0 && !a) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
  if (s > 0 && needs_arg && !arg && arg_read)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": min and max need the arg buffer");
  const int64_t nfb = (f + 63) / 64;
  if (s * nfb > (int64_t)INT32_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": too many segments");
  return 0;
}

template <typename T>
int segment_forward(const char* who, const T* src, int64_t m, int64_t f, const int64_t* indptr, int64_t s, int32_t reduce,
                    T* out, int64_t* arg, void* hip_stream) {
  if (int rc = check_pointers<T>(who, {src, out})) return rc;
  if (int rc = check_segment(who, src, out, indptr, m, f, s, reduce, arg, true)) return rc;
  if (s == 0) return 0;
  const int64_t nfb = (f + 63) / 64;
  const bool minmax = reduce == GCS_MIN || reduce == GCS_MAX;
  k_seg_fwd<T><<<(unsigned)(s * nfb), 64, 0, (hipStream_t)hip_stream>>>(src, m, f, indptr, nfb, reduce, out,
                                                                        minmax ? arg : nullptr);
  HIP_TRY(hipGetLastError(), "segment_csr forward launch");
  return 0;
}

template <typename T>
int segment_backward(const char* who, const T* dout, int64_t m, int64_t f, const int64_t* indptr, int64_t s, int32_t reduce,
                     const int64_t* arg, T* dsrc, void* hip_stream) {
  if (int rc = check_pointers<T>(who, {dout, dsrc})) return rc;
  if (int rc = check_segment(who, dsrc, dout, indptr, m, f, s, reduce, arg, true)) return rc;
  if (m == 0) return 0;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(dsrc, 0, sizeof(T) * (size_t)m * f, st), "dsrc clear");
  if (s > 0) {
    const int64_t nfb = (f + 63) / 64;
    k_seg_bwd<T><<<(unsigned)(s * nfb), 64, 0, st>>>(dout, m, f, indptr, nfb, reduce, arg, dsrc);
  }
  HIP_TRY(hipGetLastError(), "segment_csr backward launch");
  return 0;
}

}  // namespace

#include "gcs_index.h"
#include "gcs_pool.h"

namespace {

// The argument checks of gcs_serialize that need no pointer; `orders` receives the checked list.
int check_serialize(const char* who, int64_t n, int32_t n_batches, int32_t depth, const int32_t* orders_host,
                    int32_t n_orders, IndexOrders* orders) {
  const std::string w(who);
  if (n < 0 || n > INT32_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": n must be in 0...2^31 - 1");
  if (n_orders < 1 || n_orders > IX_ORDERS) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": n_orders must be in 1...5");
  if (!orders) return 0;
  if (depth < 1 || depth > 16) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": depth must be in 1...16");
  if (n_batches < 1) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": n_batches must be positive");
  int bit_length = 0;
  while (n_batches >> bit_length) bit_length++;
  if (3 * depth + bit_length > 63)
    return fail(GCS_ERR_INVALID_ARGUMENT, w + ": 3 * depth + bit_length(n_batches) exceeds 63 bits");
  if (!orders_host) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": null orders_host");
  orders->n = n_orders;
  uint32_t seen = 0;
  for (int o = 0; o < n_orders; o++) {
    const int32_t v = orders_host[o];
    if (v < 0 || v >= IX_ORDERS) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": unknown order in orders_host");
    if (seen >> v & 1u) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": repeated order in orders_host");
    seen |= 1u << v;
    orders->v[o] = v;
  }
  return 0;
}

int check_patch_plan(const char* who, const int64_t* offset, int32_t n_batches, int64_t patch_size) {
  const std::string w(who);
  if (n_batches < 1) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": n_batches must be positive");
  if (patch_size < 1) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": patch_size must be positive");
  if (!offset) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": null offset");
  return 0;
}

// The argument checks that gcs_pool_plan_workspace_bytes (which has no shift), _count and _emit share.
int check_pool_plan(const char* who, int64_t n, int32_t k, int32_t shift, bool has_shift = true) {
  const std::string w(who);
  if (n < 1 || n > INT32_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": n must be in 1...2^31 - 1");
  if (k < 1 || k > IX_ORDERS) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": k must be in 1...5 order rows");
  if (has_shift && (shift < 0 || shift > 48 || shift % 3))
    return fail(GCS_ERR_INVALID_ARGUMENT, w + ": shift must be 3 * pooling_depth in 0...48");
  return 0;
}
int check_pool_workspace(const char* who, int64_t n, int32_t k, const void* workspace, size_t workspace_bytes) {
  if (!workspace || workspace_bytes < pool_layout(n, k).total || (uintptr_t)workspace % 8)
    return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": workspace missing, not 8-byte aligned or smaller than gcs_pool_plan_workspace_bytes");
  return 0;
}

// The checks of the gathered reduce's three entry points: sizes, the reduce, and typed pointers aligned to their element.
template <typename T>
int check_gather(const char* who, int64_t m, int64_t f, int64_t s, int64_t stride, int32_t reduce,
                 std::initializer_list<const void*> typed, std::initializer_list<const void*> index) {
  const std::string w(who);
  if (m < 1 || m > INT32_MAX || s < 1 || s > INT32_MAX || f < 1 || f > INT32_MAX)
    return fail(GCS_ERR_INVALID_ARGUMENT, w + ": sizes out of range (m, s and f in 1...2^31 - 1)");
  if (stride < f) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": row stride smaller than f");
  if (reduce < GCS_SUM || reduce > GCS_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": unknown reduce");
  for (const void* p : typed)
    if (!p) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": null pointer");
  for (const void* p : index)
    if (!p || (uintptr_t)p % 8) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": null or misaligned index pointer");
  for (const void* p : typed)
    if ((uintptr_t)p % sizeof(T)) return fail(GCS_ERR_INVALID_ARGUMENT, w + ": a typed pointer is not aligned to its element");
  return 0;
}

template <typename T>
int gather_forward(const char* who, const T* src, int64_t stride, int64_t m, int64_t f, const int64_t* indices,
                   const int64_t* indptr, int64_t s, int32_t reduce, T* out, int64_t* arg, void* hip_stream) {
  if (int rc = check_gather<T>(who, m, f, s, stride, reduce, {src, out}, {indices, indptr})) return rc;
  const bool minmax = reduce == GCS_MIN || reduce == GCS_MAX;
  if (minmax && (!arg || (uintptr_t)arg % 8)) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": min and max need the arg buffer");
  hipStream_t st = (hipStream_t)hip_stream;
  constexpr int V = 16 / sizeof(T);
  if (gather_vector<T>(f, {stride}, {src, out}))
    k_gather_fwd<T, V><<<gather_blocks(s * (f / V)), GP_THREADS, 0, st>>>(src, stride, m, f, indices, indptr, s, reduce, out,
                                                                          minmax ? arg : nullptr);
  else
    k_gather_fwd<T, 1><<<gather_blocks(s * f), GP_THREADS, 0, st>>>(src, stride, m, f, indices, indptr, s, reduce, out,
                                                                    minmax ? arg : nullptr);
  HIP_TRY(hipGetLastError(), "gathered segment forward launch");
  return 0;
}

template <typename T>
int gather_backward(const char* who, const T* dout, int64_t m, int64_t f, const int64_t* cluster, const int64_t* indptr,
                    int64_t s, int32_t reduce, const int64_t* arg, T* dsrc, int64_t stride, void* hip_stream) {
  if (int rc = check_gather<T>(who, m, f, s, stride, reduce, {dout, dsrc}, {cluster, indptr})) return rc;
  const bool minmax = reduce == GCS_MIN || reduce == GCS_MAX;
  if (minmax && (!arg || (uintptr_t)arg % 8)) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": min and max need the arg buffer");
  hipStream_t st = (hipStream_t)hip_stream;
  constexpr int V = 16 / sizeof(T);
  if (gather_vector<T>(f, {stride}, {dout, dsrc}))
    k_gather_bwd<T, V><<<gather_blocks(m * (f / V)), GP_THREADS, 0, st>>>(dout, m, f, cluster, indptr, s, reduce, arg, dsrc, stride);
  else
    k_gather_bwd<T, 1><<<gather_blocks(m * f), GP_THREADS, 0, st>>>(dout, m, f, cluster, indptr, s, reduce, arg, dsrc, stride);
  HIP_TRY(hipGetLastError(), "gathered segment backward launch");
  return 0;
}

template <typename T>
int expand_add(const char* who, const T* a, const T* b, const int64_t* cluster, int64_t m, int64_t f, T* out,
               void* hip_stream) {
  if (int rc = check_gather<T>(who, m, f, 1, f, GCS_SUM, {b, out}, {cluster})) return rc;
  if ((uintptr_t)a % sizeof(T)) return fail(GCS_ERR_INVALID_ARGUMENT, std::string(who) + ": a typed pointer is not aligned to its element");
  hipStream_t st = (hipStream_t)hip_stream;
  constexpr int V = 16 / sizeof(T);
  if (gather_vector<T>(f, {}, {a, b, out}))
    k_expand_add<T, V><<<gather_blocks(m * (f / V)), GP_THREADS, 0, st>>>(a, b, cluster, m, f, out);
  else
    k_expand_add<T, 1><<<gather_blocks(m * f), GP_THREADS, 0, st>>>(a, b, cluster, m, f, out);
  HIP_TRY(hipGetLastError(), "expand add launch");
  return 0;
}

}  // namespace

extern "C" {

int gcs_index_orders(void) { return (1 << IX_ORDERS) - 1; }

size_t gcs_serialize_workspace_bytes(int64_t n, int32_t n_orders) {
  if (check_serialize("gcs_serialize_workspace_bytes", n, 1, 1, nullptr, n_orders, nullptr)) return 0;
  return index_layout(n, n_orders).total;
}

int gcs_serialize(const int32_t* grid_coord, const int64_t* batch, int64_t n, int32_t n_batches, int32_t depth,
                  float cord_div_x, float cord_div_y, const int32_t* orders_host, int32_t n_orders, int64_t* code,
                  int64_t* order, int64_t* inverse, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const char* who = "gcs_serialize";
  IndexOrders orders = {};
  if (int rc = check_serialize(who, n, n_batches, depth, orders_host, n_orders, &orders)) return rc;
  if (cord_div_x != cord_div_x || cord_div_y != cord_div_y || cord_div_x == 0.0f || cord_div_y == 0.0f)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_serialize: cord_div_x and cord_div_y must be non-zero numbers");
  if (!workspace || workspace_bytes < index_layout(n, n_orders).total)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_serialize: workspace missing or smaller than gcs_serialize_workspace_bytes");
  if (n == 0) return 0;
  if (!grid_coord) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_serialize: null grid_coord");
  if (!code || !order || !inverse) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_serialize: null code, order or inverse");
  HIP_TRY(index_serialize_launch(grid_coord, batch, n, depth, cord_div_x, cord_div_y, orders, code, order, inverse,
                                 (char*)workspace, (hipStream_t)hip_stream), "serialize launch");
  return 0;
}

int gcs_patch_plan_count(const int64_t* offset, int32_t n_batches, int64_t patch_size, int64_t counts_host[2],
                         void* hip_stream) {
  if (int rc = check_patch_plan("gcs_patch_plan_count", offset, n_batches, patch_size)) return rc;
  if (!counts_host) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_patch_plan_count: null counts_host");
  void* counts = nullptr;
  if (hipHostGetDevicePointer(&counts, counts_host, 0) != hipSuccess || !counts) {
    (void)hipGetLastError();
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_patch_plan_count: counts_host must be pinned host memory (the kernel writes it)");
  }
  hipStream_t st = (hipStream_t)hip_stream;
  k_patch_count<<<1, IX_THREADS, 0, st>>>(offset, n_batches, patch_size, (int64_t*)counts);
  HIP_TRY(hipGetLastError(), "patch count launch");
  HIP_TRY(hipStreamSynchronize(st), "patch count wait");
  return 0;
}

int gcs_patch_plan_emit(const int64_t* offset, int32_t n_batches, int64_t patch_size, int64_t padded, int64_t n_cu,
                        int64_t* pad, int64_t* unpad, int32_t* cu_seqlens, void* hip_stream) {
  if (int rc = check_patch_plan("gcs_patch_plan_emit", offset, n_batches, patch_size)) return rc;
  if (padded < 0 || padded > INT32_MAX) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_patch_plan_emit: padded must be in 0...2^31 - 1 (cu_seqlens is int32)");
  if (n_cu < 1 || n_cu > padded + n_batches + 1) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_patch_plan_emit: n_cu is not a count of gcs_patch_plan_count");
  if (!cu_seqlens || (padded > 0 && (!pad || !unpad)))
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_patch_plan_emit: null pad, unpad or cu_seqlens");
  // slices of a batch's rows: about 4 rows a thread at an even split, so that one long batch still fills the device
  int64_t slices = padded / ((int64_t)n_batches * IX_THREADS * 4) + 1;
  if (slices > 256) slices = 256;
  k_patch_emit<<<dim3((unsigned)n_batches, (unsigned)slices), IX_THREADS, 0, (hipStream_t)hip_stream>>>(
      offset, n_batches, patch_size, padded, n_cu, pad, unpad, cu_seqlens);
  HIP_TRY(hipGetLastError(), "patch emit launch");
  return 0;
}

int gcs_pool_reduces(void) { return (1 << GCS_SUM) | (1 << GCS_MEAN) | (1 << GCS_MIN) | (1 << GCS_MAX); }

size_t gcs_pool_plan_workspace_bytes(int64_t n, int32_t k) {
  if (check_pool_plan("gcs_pool_plan_workspace_bytes", n, k, 0, false)) return 0;
  return pool_layout(n, k).total;
}

int gcs_pool_plan_count(const int64_t* code, int32_t k, int64_t n, int32_t shift, void* workspace, size_t workspace_bytes,
                        int64_t counts_host[1], void* hip_stream) {
  const char* who = "gcs_pool_plan_count";
  if (int rc = check_pool_plan(who, n, k, shift)) return rc;
  if (!code) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_count: null code");
  if (int rc = check_pool_workspace(who, n, k, workspace, workspace_bytes)) return rc;
  if (!counts_host) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_count: null counts_host");
  void* counts = nullptr;
  if (hipHostGetDevicePointer(&counts, counts_host, 0) != hipSuccess || !counts) {
    (void)hipGetLastError();
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_count: counts_host must be pinned host memory (the kernel writes it)");
  }
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(pool_count_launch(code, n, k, shift, (char*)workspace, (int64_t*)counts, st), "pool plan count launch");
  HIP_TRY(hipStreamSynchronize(st), "pool plan count wait");
  return 0;
}

int gcs_pool_plan_emit(const int64_t* code, int32_t k, int64_t n, int32_t shift, int64_t s, void* workspace,
                       size_t workspace_bytes, int64_t* cluster, int64_t* indices, int64_t* idx_ptr, int64_t* head,
                       int64_t* down_code, int64_t* down_order, int64_t* down_inverse, void* hip_stream) {
  const char* who = "gcs_pool_plan_emit";
  if (int rc = check_pool_plan(who, n, k, shift)) return rc;
  if (s < 1 || s > n) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_emit: s is not a count of gcs_pool_plan_count (1...n)");
  if (!code) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_emit: null code");
  if (int rc = check_pool_workspace(who, n, k, workspace, workspace_bytes)) return rc;
  if (!cluster || !indices || !idx_ptr || !head || !down_code || !down_order || !down_inverse)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_pool_plan_emit: null cluster, indices, idx_ptr, head, down_code, down_order or down_inverse");
  HIP_TRY(pool_emit_launch(code, n, k, shift, s, (char*)workspace, cluster, indices, idx_ptr, head, down_code, down_order,
                           down_inverse, (hipStream_t)hip_stream), "pool plan emit launch");
  return 0;
}

int gcs_segment_gather_forward_t(int32_t dtype, const void* src, int64_t src_stride, int64_t m, int64_t f,
                                 const int64_t* indices, const int64_t* indptr, int64_t s, int32_t reduce, void* out,
                                 int64_t* arg, void* hip_stream) {
  const char* who = "gcs_segment_gather_forward_t";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (dtype == GCS_F32)
    return gather_forward(who, (const float*)src, src_stride, m, f, indices, indptr, s, reduce, (float*)out, arg, hip_stream);
  return gather_forward(who, (const half_t*)src, src_stride, m, f, indices, indptr, s, reduce, (half_t*)out, arg, hip_stream);
}

int gcs_segment_gather_backward_t(int32_t dtype, const void* dout, int64_t m, int64_t f, const int64_t* cluster,
                                  const int64_t* indptr, int64_t s, int32_t reduce, const int64_t* arg, void* dsrc,
                                  int64_t dsrc_stride, void* hip_stream) {
  const char* who = "gcs_segment_gather_backward_t";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (dtype == GCS_F32)
    return gather_backward(who, (const float*)dout, m, f, cluster, indptr, s, reduce, arg, (float*)dsrc, dsrc_stride, hip_stream);
  return gather_backward(who, (const half_t*)dout, m, f, cluster, indptr, s, reduce, arg, (half_t*)dsrc, dsrc_stride, hip_stream);
}

int gcs_segment_expand_add_t(int32_t dtype, const void* a, const void* b, const int64_t* cluster, int64_t m, int64_t f,
                             void* out, void* hip_stream) {
  const char* who = "gcs_segment_expand_add_t";
  if (int rc = check_dtype(who, dtype)) return rc;
  if (dtype == GCS_F32) return expand_add(who, (const float*)a, (const float*)b, cluster, m, f, (float*)out, hip_stream);
  return expand_add(who, (const half_t*)a, (const half_t*)b, cluster, m, f, (half_t*)out, hip_stream);
}

int gcs_abi_version(void) { return GCS_ABI_VERSION; }
const char* gcs_last_error(void) { return g_err.c_str(); }

size_t gcs_subm_rulebook_bytes(int64_t n, int32_t kvol) {
  if (check_conv_dims("gcs_subm_rulebook_bytes", n, kvol, 1, 1)) return 0;
  return carve_rulebook(nullptr, n, kvol).bytes;
}
size_t gcs_subm_rulebook_scratch_bytes(int64_t n) {
  if (check_conv_dims("gcs_subm_rulebook_scratch_bytes", n, 1, 1, 1)) return 0;
  return carve_scratch(nullptr, n).bytes;
}
size_t gcs_subm_backward_workspace_bytes(int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups) {
  if (check_conv_dims("gcs_subm_backward_workspace_bytes", n, kvol, cin, cout)) return 0;
  const EnginePlan e = engine_plan_of(GCS_ENGINE_VALU, n, cin, cout, kvol);
  return carve_bwd<float>(nullptr, e, n, cin, cout, kvol, dups).bytes;
}

int gcs_subm_plan(int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t plan[5]) {
  if (int rc = check_conv_dims("gcs_subm_plan", n, kvol, cin, cout)) return rc;
  if (!plan) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_plan: null plan");
  const Plan p = plan_of(n, cin, cout, kvol);
  plan[0] = p.fwd;
  plan[1] = p.dx;
  plan[2] = p.dw;
  plan[3] = p.dw_slices;
  plan[4] = p.db_slices;
  return 0;
}

int gcs_subm_rulebook(const int32_t* indices, int64_t n, int32_t batch_size, const int32_t* spatial_shape,
                      const int32_t* ksize, const int32_t* dilation, void* rulebook, size_t rulebook_bytes,
                      void* scratch, size_t scratch_bytes, int32_t* host_info, void* hip_stream) {
  if (!spatial_shape || !ksize || !dilation) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: null shape argument");
  Geom g{batch_size, spatial_shape[0], spatial_shape[1], spatial_shape[2], ksize[0], ksize[1], ksize[2],
         dilation[0], dilation[1], dilation[2]};
  for (int d = 0; d < 3; d++) {
    if (ksize[d] < 1 || ksize[d] % 2 == 0)
      return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: kernel sizes must be odd and positive");
    if (dilation[d] < 1) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: dilations must be positive");
    if (spatial_shape[d] < 1) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: spatial_shape must be positive");
  }
  if (batch_size < 1) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: batch_size must be positive");
  const int32_t K = ksize[0] * ksize[1] * ksize[2];
  if (int rc = check_conv_dims("gcs_subm_rulebook", n, K, 1, 1)) return rc;
  // every packed key must stay below the empty marker: batch_size * prod(spatial_shape) <= 2^63
  unsigned __int128 vol = (unsigned __int128)(uint32_t)batch_size * (uint32_t)g.s0 * (uint32_t)g.s1 * (uint32_t)g.s2;
  if (vol > ((unsigned __int128)1 << 63))
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: batch_size * spatial_shape does not fit the 64-bit key");
  const Rulebook rb = carve_rulebook(rulebook, n, K);
  const Scratch sc = carve_scratch(scratch, n);
  if (!rulebook || rulebook_bytes < rb.bytes)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: rulebook buffer missing or smaller than gcs_subm_rulebook_bytes");
  if (!scratch || scratch_bytes < sc.bytes)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: scratch buffer missing or smaller than gcs_subm_rulebook_scratch_bytes");
  if (n > 0 && !indices) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_rulebook: null indices");
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(rb.hdr, 0, 4 * (4 + (size_t)K), st), "rulebook header clear");
  if (n > 0) {
    const uint64_t cap = table_capacity(n), mask = cap - 1;
    const int64_t nb = scan_blocks(n);
    HIP_TRY(hipMemsetAsync(sc.keys, 0xFF, 8 * cap, st), "hash key clear");
    HIP_TRY(hipMemsetAsync(sc.vals, 0x7F, 4 * cap, st), "hash value clear");
    HIP_TRY(hipMemsetAsync(rb.gcnt, 0, 4 * (size_t)n, st), "group count clear");
    HIP_TRY(hipMemsetAsync(sc.gfill, 0, 4 * (size_t)n, st), "group fill clear");
    k_insert<<<blocks_for(n, 256), 256, 0, st>>>(indices, n, g, sc.keys, sc.vals, mask, rb.hdr);
    k_neighbours<<<blocks_for(n * K, 256), 256, 0, st>>>(indices, n, g, sc.keys, sc.vals, mask, rb.nbr, rb.rep, rb.hdr);
    const dim3 gp((unsigned)nb, (unsigned)K);
    k_scan_count<0><<<gp, kScanThreads, 0, st>>>(rb.nbr, n, K, rb.hdr, sc.bsum);
    k_scan_blocks<0><<<blocks_for(K, 64), 64, 0, st>>>(sc.bsum, nb, K, rb.hdr);
    k_scan_write<0><<<gp, kScanThreads, 0, st>>>(rb.nbr, n, K, rb.hdr, sc.bsum, rb.prow);
    // duplicate groups: every kernel below returns at once when the centre taps found no duplicate
    k_group_count<<<blocks_for(n, 256), 256, 0, st>>>(rb.rep, n, rb.hdr, rb.gcnt);
    const dim3 g1((unsigned)nb, 1);
    k_scan_count<1><<<g1, kScanThreads, 0, st>>>(rb.gcnt, n, 1, rb.hdr, sc.bsum);
    k_scan_blocks<1><<<1, 64, 0, st>>>(sc.bsum, nb, 1, rb.hdr);
    k_scan_write<1><<<g1, kScanThreads, 0, st>>>(rb.gcnt, n, 1, rb.hdr, sc.bsum, rb.gstart);
    k_group_fill<<<blocks_for(n, 256), 256, 0, st>>>(rb.rep, n, rb.hdr, rb.gstart, sc.gfill, rb.glist);
    k_group_sort<<<blocks_for(n, 256), 256, 0, st>>>(n, rb.hdr, rb.gstart, rb.gcnt, rb.glist);
    HIP_TRY(hipGetLastError(), "rulebook launch");
  }
  if (host_info) {
    int32_t h[4 + kMaxK];
    HIP_TRY(hipMemcpyAsync(h, rb.hdr, 4 * (4 + (size_t)K), hipMemcpyDeviceToHost, st), "rulebook header read-back");
    HIP_TRY(hipStreamSynchronize(st), "rulebook wait");
    host_info[0] = h[0];
    host_info[1] = h[1];
    for (int k = 0; k < K; k++) host_info[GCS_HOST_INFO_HEADER + k] = h[4 + k];
  }
  return 0;
}

int gcs_subm_forward(const void* rulebook, int64_t n, int32_t kvol, const float* features, int32_t cin,
                     const float* weight, const float* bias, int32_t cout, float* out, void* hip_stream) {
  return subm_forward("gcs_subm_forward", route_f32(GCS_ENGINE_VALU), rulebook, n, kvol, features, cin, weight, bias, cout, out, nullptr,
                      0, hip_stream);
}
int gcs_subm_forward_engine(int32_t engine, const void* rulebook, int64_t n, int32_t kvol, const float* features,
                            int32_t cin, const float* weight, const float* bias, int32_t cout, float* out,
                            void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rc = check_engine("gcs_subm_forward_engine", engine)) return rc;
  return subm_forward("gcs_subm_forward_engine", route_f32(engine), rulebook, n, kvol, features, cin, weight, bias, cout, out, workspace,
                      workspace_bytes, hip_stream);
}

int gcs_subm_backward(const void* rulebook, int64_t n, int32_t kvol, int32_t dups, const float* features,
                      int32_t cin, const float* weight, int32_t cout, const float* dout, float* dx, float* dw,
                      float* db, void* workspace, size_t workspace_bytes, void* hip_stream) {
  return subm_backward("gcs_subm_backward", route_f32(GCS_ENGINE_VALU), rulebook, n, kvol, dups, features, cin, weight, cout, dout, dx, dw,
                       db, workspace, workspace_bytes, hip_stream);
}
int gcs_subm_backward_engine(int32_t engine, const void* rulebook, int64_t n, int32_t kvol, int32_t dups,
                             const float* features, int32_t cin, const float* weight, int32_t cout, const float* dout,
                             float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rc = check_engine("gcs_subm_backward_engine", engine)) return rc;
  return subm_backward("gcs_subm_backward_engine", route_f32(engine), rulebook, n, kvol, dups, features, cin, weight, cout, dout, dx, dw,
                       db, workspace, workspace_bytes, hip_stream);
}

int gcs_subm_engine_plan(int32_t engine, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t plan[7]) {
  if (int rc = check_engine("gcs_subm_engine_plan", engine)) return rc;
  if (int rc = check_conv_dims("gcs_subm_engine_plan", n, kvol, cin, cout)) return rc;
  if (!plan) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_engine_plan: null plan");
  const EnginePlan e = engine_plan_of(engine, n, cin, cout, kvol);
  plan[0] = e.p.fwd;
  plan[1] = e.p.dx;
  plan[2] = e.p.dw;
  plan[3] = e.p.dw_slices;
  plan[4] = e.p.db_slices;
  plan[5] = e.fwd_slices;
  plan[6] = e.dx_slices;
  return 0;
}
int gcs_engine_products(int32_t engine) {
  if (int rc = check_engine("gcs_engine_products", engine)) return rc;
  return engine == GCS_ENGINE_MFMA ? GCS_PRODUCT_FORWARD | GCS_PRODUCT_DX | GCS_PRODUCT_DW : 0;
}
int gcs_subm_engine_workspace_bytes(int32_t engine, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups,
                                    size_t* forward_bytes, size_t* backward_bytes) {
  if (int rc = check_engine("gcs_subm_engine_workspace_bytes", engine)) return rc;
  if (int rc = check_conv_dims("gcs_subm_engine_workspace_bytes", n, kvol, cin, cout)) return rc;
  if (!forward_bytes || !backward_bytes)
    return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_engine_workspace_bytes: null output");
  const EnginePlan e = engine_plan_of(engine, n, cin, cout, kvol);
  *forward_bytes = forward_ws_bytes(e, n, cout);
  *backward_bytes = carve_bwd<float>(nullptr, e, n, cin, cout, kvol, dups).bytes;
  return 0;
}

int gcs_segment_csr_forward(const float* src, int64_t m, int64_t f, const int64_t* indptr, int64_t s, int32_t reduce,
                            float* out, int64_t* arg, void* hip_stream) {
  return segment_forward("gcs_segment_csr_forward", src, m, f, indptr, s, reduce, out, arg, hip_stream);
}
int gcs_segment_csr_backward(const float* dout, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                             int32_t reduce, const int64_t* arg, float* dsrc, void* hip_stream) {
  return segment_backward("gcs_segment_csr_backward", dout, m, f, indptr, s, reduce, arg, dsrc, hip_stream);
}

// ---- the typed entry points: GCS_F32 is the default entry points above, GCS_F16 the same host paths on half_t ------------
int gcs_dtypes(void) { return (1 << GCS_F32) | (1 << GCS_F16); }

int gcs_subm_workspace_bytes_t(int32_t dtype, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups,
                               size_t* forward_bytes, size_t* backward_bytes) {
  if (int rc = check_dtype("gcs_subm_workspace_bytes_t", dtype)) return rc;
  if (int rc = check_conv_dims("gcs_subm_workspace_bytes_t", n, kvol, cin, cout)) return rc;
  if (!forward_bytes || !backward_bytes) return fail(GCS_ERR_INVALID_ARGUMENT, "gcs_subm_workspace_bytes_t: null output");
  const EnginePlan e = engine_plan_of(dtype == GCS_F32 ? GCS_ENGINE_VALU : GCS_ENGINE_MFMA, n, cin, cout, kvol);
  *forward_bytes = forward_ws_bytes(e, n, cout);
  *backward_bytes = dtype == GCS_F32 ? carve_bwd<float>(nullptr, e, n, cin, cout, kvol, dups).bytes
                                     : carve_bwd<half_t>(nullptr, e, n, cin, cout, kvol, dups).bytes;
  return 0;
}

int gcs_subm_forward_t(int32_t dtype, const void* rulebook, int64_t n, int32_t kvol, const void* features, int32_t cin,
                       const void* weight, const void* bias, int32_t cout, void* out, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
  if (int rc = check_dtype("gcs_subm_forward_t", dtype)) return rc;
  if (dtype == GCS_F32)
    return subm_forward("gcs_subm_forward_t", route_f32(GCS_ENGINE_VALU), rulebook, n, kvol, (const float*)features, cin,
                        (const float*)weight, (const float*)bias, cout, (float*)out, nullptr, 0, hip_stream);
  return subm_forward("gcs_subm_forward_t", kRouteF16, rulebook, n, kvol, (const half_t*)features, cin, (const half_t*)weight,
                      (const half_t*)bias, cout, (half_t*)out, workspace, workspace_bytes, hip_stream);
}

int gcs_subm_backward_t(int32_t dtype, const void* rulebook, int64_t n, int32_t kvol, int32_t dups, const void* features,
                        int32_t cin, const void* weight, int32_t cout, const void* dout, void* dx, void* dw, void* db,
                        void* workspace, size_t workspace_bytes, void* hip_stream) {
  if (int rc = check_dtype("gcs_subm_backward_t", dtype)) return rc;
  if (dtype == GCS_F32)
    return subm_backward("gcs_subm_backward_t", route_f32(GCS_ENGINE_VALU), rulebook, n, kvol, dups, (const float*)features,
                         cin, (const float*)weight, cout, (const float*)dout, (float*)dx, (float*)dw, (float*)db, workspace,
                         workspace_bytes, hip_stream);
  return subm_backward("gcs_subm_backward_t", kRouteF16, rulebook, n, kvol, dups, (const half_t*)features, cin,
                       (const half_t*)weight, cout, (const half_t*)dout, (half_t*)dx, (half_t*)dw, (half_t*)db, workspace,
                       workspace_bytes, hip_stream);
}

int gcs_segment_csr_forward_t(int32_t dtype, const void* src, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                              int32_t reduce, void* out, int64_t* arg, void* hip_stream) {
  if (int rc = check_dtype("gcs_segment_csr_forward_t", dtype)) return rc;
  if (dtype == GCS_F32)
    return gcs_segment_csr_forward((const float*)src, m, f, indptr, s, reduce, (float*)out, arg, hip_stream);
  return segment_forward("gcs_segment_csr_forward_t", (const half_t*)src, m, f, indptr, s, reduce, (half_t*)out, arg,
                         hip_stream);
}

int gcs_segment_csr_backward_t(int32_t dtype, const void* dout, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                               int32_t reduce, const int64_t* arg, void* dsrc, void* hip_stream) {
  if (int rc = check_dtype("gcs_segment_csr_backward_t", dtype)) return rc;
  if (dtype == GCS_F32)
    return gcs_segment_csr_backward((const float*)dout, m, f, indptr, s, reduce, arg, (float*)dsrc, hip_stream);
  return segment_backward("gcs_segment_csr_backward_t", (const half_t*)dout, m, f, indptr, s, reduce, arg, (half_t*)dsrc,
                          hip_stream);
}

}  // extern "C"
