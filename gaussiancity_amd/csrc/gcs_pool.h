// gcs_pool.h -- SerializedPooling / SerializedUnpooling of the PTv3 point backbone (gcs_pool_plan_*, gcs_segment_gather_*,
// gcs_segment_expand_add_t, include/gcs.h): the cluster plan of a pooling stage as kernels with one host wait, and the
// row-indexed segment reduce around it, so that neither `feat[indices]` nor `feat[inverse]` is ever materialised.
// Included by gcs_sparse.hip after gcs_index.h, whose radix sort it runs; device code and launch helpers only, the C ABI
// stays in gcs_sparse.hip.  DESIGN.md section 15.6.
//
//   plan     _count: k_pool_keys writes key[j] = code[0][j] >> shift into the workspace with its 8 digit histograms, the
//            sort of gcs_index.h orders the rows by key (ties to the lower row: that order IS `indices`), k_pool_heads
//            counts the positions whose key differs from the one in front per tile of IX_TILE positions, and one block
//            (k_pool_total) scans the tile counts and writes S to the caller's pinned word.
//            _emit: k_pool_emit scans the head flags inside its tile and writes cluster, indices, idx_ptr, head and
//            down_code; row 0 of down_code is the distinct keys in ascending order, so its order and inverse are the
//            identity and written there too; k_pool_hist and the same sort give down_order / down_inverse of the other
//            order rows in the same launches (none for one order row).
//   reduce   k_gather_fwd / k_gather_bwd / k_expand_add: a work item is (segment or row, piece of V elements), V = 16 bytes
//            (4 floats, 8 halves) or one element where the width, a stride or a base address is no multiple of 16 bytes.
//            Items are dealt to threads in order, so a wave carries 64 / pieces-per-row segments and no lane idles at any
//            width; a thread walks its segment's rows in ascending j with its own fp32 chain -- a chain is never split.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------- plan
// key[j] = code[0][j] >> shift (arithmetic), and the 8 byte-digit histograms of the keys (ghist row 0)
__global__ __launch_bounds__(IX_THREADS) void k_pool_keys(const int64_t* __restrict__ code, uint32_t n, int shift,
                                                          int64_t* __restrict__ key, uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[IX_PASSES * IX_RADIX];
  const uint32_t tid = threadIdx.x;
  for (int b = tid; b < IX_PASSES * IX_RADIX; b += IX_THREADS) h[b] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * IX_TILE;
  for (int it = 0; it < IX_ITEMS; it++) {
    const uint32_t i = base + it * IX_THREADS + tid;
    if (i >= n) break;
    const int64_t c = code[i] >> shift;
    key[i] = c;
    const uint64_t u = (uint64_t)c ^ IX_SIGN;
#pragma unroll
    for (int p = 0; p < IX_PASSES; p++) atomicAdd(&h[p * IX_RADIX + (uint32_t)(u >> (p * IX_BITS) & (IX_RADIX - 1))], 1u);
  }
  __syncthreads();
  for (int b = tid; b < IX_PASSES * IX_RADIX; b += IX_THREADS)
    if (h[b]) atomicAdd(&ghist[b], h[b]);
}

// digit histograms of the rows of keys [k][n] (blockIdx.y = row) into ghist [k][IX_PASSES][IX_RADIX]
__global__ __launch_bounds__(IX_THREADS) void k_pool_hist(const int64_t* __restrict__ keys, uint32_t n,
                                                          uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[IX_PASSES * IX_RADIX];
  const uint32_t tid = threadIdx.x;
  for (int b = tid; b < IX_PASSES * IX_RADIX; b += IX_THREADS) h[b] = 0;
  __syncthreads();
  const int64_t* row = keys + (size_t)blockIdx.y * n;
  const uint32_t base = blockIdx.x * IX_TILE;
  for (int it = 0; it < IX_ITEMS; it++) {
    const uint32_t i = base + it * IX_THREADS + tid;
    if (i >= n) break;
    const uint64_t u = (uint64_t)row[i] ^ IX_SIGN;
#pragma unroll
    for (int p = 0; p < IX_PASSES; p++) atomicAdd(&h[p * IX_RADIX + (uint32_t)(u >> (p * IX_BITS) & (IX_RADIX - 1))], 1u);
  }
  __syncthreads();
  uint32_t* g = ghist + (size_t)blockIdx.y * IX_PASSES * IX_RADIX;
  for (int b = tid; b < IX_PASSES * IX_RADIX; b += IX_THREADS)
    if (h[b]) atomicAdd(&g[b], h[b]);
}

// the row at sorted position p; a value outside [0, n) cannot come out of the sort and reads row 0
__device__ __forceinline__ uint32_t pool_row(const int64_t* __restrict__ sorted, uint32_t p, uint32_t n) {
  const uint64_t r = (uint64_t)sorted[p];
  return r < n ? (uint32_t)r : 0u;
}
// position p opens a cluster: its key differs from the key one position in front
__device__ __forceinline__ bool pool_head(const int64_t* __restrict__ key, const int64_t* __restrict__ sorted, uint32_t p,
                                          uint32_t n) {
  return p == 0 || key[pool_row(sorted, p, n)] != key[pool_row(sorted, p - 1, n)];
}

// heads per tile of IX_TILE positions -> tiles[blockIdx.x]
__global__ __launch_bounds__(IX_THREADS) void k_pool_heads(const int64_t* __restrict__ key,
                                                           const int64_t* __restrict__ sorted, uint32_t n,
                                                           uint32_t* __restrict__ tiles) {
  __shared__ uint32_t lds4[4];
  const uint32_t base = blockIdx.x * IX_TILE;
  uint32_t c = 0;
  for (int it = 0; it < IX_ITEMS; it++) {
    const uint32_t p = base + it * IX_THREADS + threadIdx.x;
    if (p < n && pool_head(key, sorted, p, n)) c++;
  }
  uint32_t total;
  ix_block_excl_scan(c, lds4, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// one block: exclusive scan of the tile counts in place, the total to the caller's pinned word
__global__ __launch_bounds__(IX_THREADS) void k_pool_total(uint32_t* __restrict__ tiles, uint32_t nb, int64_t* counts) {
  __shared__ uint32_t lds4[4];
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += IX_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? tiles[i] : 0u;
    uint32_t total;
    const uint32_t ex = ix_block_excl_scan(v, lds4, &total);
    if (i < nb) tiles[i] = running + ex;
    running += total;
  }
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)running;
    __threadfence_system();
  }
}

// A block per tile of IX_TILE sorted positions, a thread per IX_ITEMS consecutive ones: the cluster number of a position
// is the number of heads up to it, minus one.  Row 0 of down_order / down_inverse is the identity and written here; the other
// order rows are sorted afterwards.  Every store is held inside n, s and k * s.
__global__ __launch_bounds__(IX_THREADS) void k_pool_emit(const int64_t* __restrict__ code, int k, uint32_t n, int shift,
                                                          uint32_t s, const int64_t* __restrict__ key,
                                                          const int64_t* __restrict__ sorted,
                                                          const uint32_t* __restrict__ tiles, int64_t* __restrict__ cluster,
                                                          int64_t* __restrict__ indices, int64_t* __restrict__ idx_ptr,
                                                          int64_t* __restrict__ head, int64_t* __restrict__ down_code,
                                                          int64_t* __restrict__ down_order,
                                                          int64_t* __restrict__ down_inverse) {
  __shared__ uint32_t lds4[4];
  const uint32_t first = blockIdx.x * IX_TILE + threadIdx.x * IX_ITEMS;
  uint32_t flags = 0, c = 0;
#pragma unroll
  for (int i = 0; i < IX_ITEMS; i++) {
    const uint32_t p = first + i;
    if (p < n && pool_head(key, sorted, p, n)) {
      flags |= 1u << i;
      c++;
    }
  }
  uint32_t total;
  uint32_t seen = tiles[blockIdx.x] + ix_block_excl_scan(c, lds4, &total);  // heads in front of this thread's positions
#pragma unroll
  for (int i = 0; i < IX_ITEMS; i++) {
    const uint32_t p = first + i;
    if (p >= n) break;
    const uint32_t row = pool_row(sorted, p, n);
    const bool is_head = flags >> i & 1u;
    seen += is_head;
    const uint32_t cl = seen - 1;  // seen >= 1: position 0 is a head
    indices[p] = (int64_t)row;
    if (cl >= s) continue;  // a count that does not belong to this workspace
    cluster[row] = (int64_t)cl;
    if (is_head) {
      idx_ptr[cl] = (int64_t)p;
      head[cl] = (int64_t)row;
      for (int r = 0; r < k; r++) down_code[(size_t)r * s + cl] = code[(size_t)r * n + row] >> shift;
      down_order[cl] = (int64_t)cl;  // row 0 of down_code is the distinct keys in ascending order: already sorted
      down_inverse[cl] = (int64_t)cl;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) idx_ptr[s] = (int64_t)n;
}

struct PoolLayout {
  IndexLayout sort;  // the sort's share, sized for k rows of n keys: _count sorts one row of n, _emit k rows of s <= n
  size_t key, sorted, inverse, tiles, total;
};
inline PoolLayout pool_layout(int64_t n, int32_t k) {
  PoolLayout lay;
  lay.sort = index_layout(n, k);
  size_t o = lay.sort.total;
  lay.key = o;     o += align_up(sizeof(int64_t) * (size_t)n);
  lay.sorted = o;  o += align_up(sizeof(int64_t) * (size_t)n);
  lay.inverse = o; o += align_up(sizeof(int64_t) * (size_t)n);
  lay.tiles = o;   o += align_up(sizeof(uint32_t) * (size_t)lay.sort.nb);
  lay.total = o;
  return lay;
}

// the sort of gcs_index.h over keys [rows][n] whose digit histograms are in s.ghist: plan, then 8 passes
inline void pool_sort_launch(const int64_t* keys, int64_t n, int32_t rows, const IndexLayout& lay, const IndexSort& s,
                             int64_t* order, int64_t* inverse, hipStream_t st) {
  k_index_plan<<<rows, IX_THREADS, 0, st>>>(s.ghist, (uint32_t)n, s.plan);
  const dim3 tiles(lay.nb, rows), digits(IX_RADIX, rows);
  const bool scanned = lay.nb > IX_SCAN_MIN_BLOCKS;
  for (int p = 0; p < IX_PASSES; p++) {
    k_index_radix_hist<<<tiles, IX_THREADS, 0, st>>>(keys, (uint32_t)n, p, lay.nb, s);
    if (scanned) k_index_radix_scan<<<digits, IX_THREADS, 0, st>>>(p, lay.nb, s);
    k_index_radix_scatter<<<tiles, IX_THREADS, 0, st>>>(keys, (uint32_t)n, p, lay.nb, scanned, s, order, inverse);
  }
}
inline IndexSort pool_sort_buffers(char* ws, const IndexLayout& lay) {
  IndexSort s;
  s.rows[0] = (uint32_t*)(ws + lay.rows[0]);
  s.rows[1] = (uint32_t*)(ws + lay.rows[1]);
  s.table = (uint32_t*)(ws + lay.table);
  s.ghist = (uint32_t*)(ws + lay.ghist);
  s.plan = (uint32_t*)(ws + lay.plan);
  return s;
}

// arguments checked; counts is the device view of the caller's pinned word
inline hipError_t pool_count_launch(const int64_t* code, int64_t n, int32_t k, int shift, char* ws, int64_t* counts,
                                    hipStream_t st) {
  const PoolLayout lay = pool_layout(n, k);
  const IndexLayout one = index_layout(n, 1);
  const IndexSort s = pool_sort_buffers(ws, one);
  int64_t* key = (int64_t*)(ws + lay.key);
  int64_t* sorted = (int64_t*)(ws + lay.sorted);
  uint32_t* tiles = (uint32_t*)(ws + lay.tiles);
  hipError_t e = hipMemsetAsync(s.ghist, 0, sizeof(uint32_t) * IX_PASSES * IX_RADIX, st);
  if (e != hipSuccess) return e;
  k_pool_keys<<<one.nb, IX_THREADS, 0, st>>>(code, (uint32_t)n, shift, key, s.ghist);
  pool_sort_launch(key, n, 1, one, s, sorted, (int64_t*)(ws + lay.inverse), st);
  k_pool_heads<<<one.nb, IX_THREADS, 0, st>>>(key, sorted, (uint32_t)n, tiles);
  k_pool_total<<<1, IX_THREADS, 0, st>>>(tiles, one.nb, counts);
  return hipGetLastError();
}

inline hipError_t pool_emit_launch(const int64_t* code, int64_t n, int32_t k, int shift, int64_t s_, char* ws,
                                   int64_t* cluster, int64_t* indices, int64_t* idx_ptr, int64_t* head, int64_t* down_code,
                                   int64_t* down_order, int64_t* down_inverse, hipStream_t st) {
  const PoolLayout lay = pool_layout(n, k);
  const uint32_t nb = lay.sort.nb;
  k_pool_emit<<<nb, IX_THREADS, 0, st>>>(code, k, (uint32_t)n, shift, (uint32_t)s_, (const int64_t*)(ws + lay.key),
                                         (const int64_t*)(ws + lay.sorted), (const uint32_t*)(ws + lay.tiles), cluster,
                                         indices, idx_ptr, head, down_code, down_order, down_inverse);
  if (k == 1) return hipGetLastError();
  const int32_t rest = k - 1;  // the order rows that still need their sort
  const IndexLayout down = index_layout(s_, rest);  // inside the sort's share: every part of it grows with n and k
  const IndexSort s = pool_sort_buffers(ws, down);
  hipError_t e = hipMemsetAsync(s.ghist, 0, sizeof(uint32_t) * IX_PASSES * IX_RADIX * rest, st);
  if (e != hipSuccess) return e;
  k_pool_hist<<<dim3(down.nb, rest), IX_THREADS, 0, st>>>(down_code + s_, (uint32_t)s_, s.ghist);
  pool_sort_launch(down_code + s_, s_, rest, down, s, down_order + s_, down_inverse + s_, st);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------- gathered reduce
constexpr int GP_THREADS = 256;
constexpr unsigned GP_MAX_BLOCKS = 2048;  // 8 workgroups a CU; beyond, the grid strides

template <typename T, int V>
struct alignas(sizeof(T) * V) Piece {
  T v[V];
};

// item = (segment c, piece q of the row).  Sum and mean: one fp32 chain from 0 in ascending j, mean divided in fp32, one
// conversion to T.  Min and max compare as k_seg_fwd does and copy bits; arg is the SOURCE row of the first j that
// attains the value.  A row outside [0, m) is not a precondition's row: it is skipped, never read.
template <typename T, int V>
__global__ __launch_bounds__(GP_THREADS) void k_gather_fwd(const T* __restrict__ src, int64_t stride, int64_t m, int64_t f,
                                                           const int64_t* __restrict__ indices,
                                                           const int64_t* __restrict__ indptr, int64_t s, int reduce,
                                                           T* __restrict__ out, int64_t* __restrict__ arg) {
  using P = Piece<T, V>;
  const int64_t pieces = f / V, items = s * pieces;
  for (int64_t it = (int64_t)blockIdx.x * GP_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * GP_THREADS) {
    const int64_t c = it / pieces, col = (it - c * pieces) * V;
    int64_t lo, hi;
    seg_bounds(indptr, c, m, &lo, &hi);
    P res;
    int64_t best[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
      res.v[e] = (T)0.0f;
      best[e] = -1;
    }
    if (reduce == GCS_SUM || reduce == GCS_MEAN) {
      float acc[V];
#pragma unroll
      for (int e = 0; e < V; e++) acc[e] = 0.0f;
      for (int64_t j = lo; j < hi; j++) {
        const int64_t r = indices[j];
        if ((uint64_t)r >= (uint64_t)m) continue;
        const P x = *(const P*)(src + r * stride + col);
#pragma unroll
        for (int e = 0; e < V; e++) acc[e] += (float)x.v[e];
      }
      const float cnt = (float)(hi - lo);
#pragma unroll
      for (int e = 0; e < V; e++) res.v[e] = (T)((reduce == GCS_MEAN && hi > lo) ? acc[e] / cnt : acc[e]);
    } else {
      for (int64_t j = lo; j < hi; j++) {
        const int64_t r = indices[j];
        if ((uint64_t)r >= (uint64_t)m) continue;
        const P x = *(const P*)(src + r * stride + col);
#pragma unroll
        for (int e = 0; e < V; e++) {
          const bool better = reduce == GCS_MAX ? (float)x.v[e] > (float)res.v[e] : (float)x.v[e] < (float)res.v[e];
          if (best[e] < 0 || better) {
            res.v[e] = x.v[e];
            best[e] = r;
          }
        }
      }
    }
    *(P*)(out + c * f + col) = res;
    if (arg) {
#pragma unroll
      for (int e = 0; e < V; e++) arg[c * f + col + e] = best[e];
    }
  }
}

// item = (row r, piece q): the transpose by row.  Every element of dsrc is written exactly once.
template <typename T, int V>
__global__ __launch_bounds__(GP_THREADS) void k_gather_bwd(const T* __restrict__ dout, int64_t m, int64_t f,
                                                           const int64_t* __restrict__ cluster,
                                                           const int64_t* __restrict__ indptr, int64_t s, int reduce,
                                                           const int64_t* __restrict__ arg, T* __restrict__ dsrc,
                                                           int64_t stride) {
  using P = Piece<T, V>;
  const int64_t pieces = f / V, items = m * pieces;
  for (int64_t it = (int64_t)blockIdx.x * GP_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * GP_THREADS) {
    const int64_t r = it / pieces, col = (it - r * pieces) * V;
    const int64_t c = cluster[r];
    P g;
#pragma unroll
    for (int e = 0; e < V; e++) g.v[e] = (T)0.0f;
    if ((uint64_t)c < (uint64_t)s) {  // a row of no segment gets zeros
      g = *(const P*)(dout + c * f + col);
      if (reduce == GCS_MEAN) {
        int64_t lo, hi;
        seg_bounds(indptr, c, m, &lo, &hi);
        if (hi > lo) {
          const float cnt = (float)(hi - lo);
#pragma unroll
          for (int e = 0; e < V; e++) g.v[e] = (T)((float)g.v[e] / cnt);
        }
      } else if (reduce == GCS_MIN || reduce == GCS_MAX) {
#pragma unroll
        for (int e = 0; e < V; e++)
          if (arg[c * f + col + e] != r) g.v[e] = (T)0.0f;
      }
    }
    *(P*)(dsrc + r * stride + col) = g;
  }
}

// out[r] = a[r] + b[cluster[r]]: one fp32 add, rounded once; without a, b's bits
template <typename T, int V>
__global__ __launch_bounds__(GP_THREADS) void k_expand_add(const T* __restrict__ a, const T* __restrict__ b,
                                                           const int64_t* __restrict__ cluster, int64_t m, int64_t f,
                                                           T* __restrict__ out) {
  using P = Piece<T, V>;
  const int64_t pieces = f / V, items = m * pieces;
  for (int64_t it = (int64_t)blockIdx.x * GP_THREADS + threadIdx.x; it < items; it += (int64_t)gridDim.x * GP_THREADS) {
    const int64_t r = it / pieces, col = (it - r * pieces) * V;
    P y = *(const P*)(b + cluster[r] * f + col);
    if (a) {
      const P x = *(const P*)(a + r * f + col);
#pragma unroll
      for (int e = 0; e < V; e++) y.v[e] = (T)((float)x.v[e] + (float)y.v[e]);
    }
    *(P*)(out + r * f + col) = y;
  }
}

// 16-byte pieces when the width, every stride and every base address allow them
template <typename T>
bool gather_vector(int64_t f, std::initializer_list<int64_t> strides, std::initializer_list<const void*> bases) {
  constexpr int64_t V = 16 / sizeof(T);
  if (f % V) return false;
  for (int64_t st : strides)
    if (st % V) return false;
  for (const void* p : bases)
    if ((uintptr_t)p % 16) return false;
  return true;
}
inline unsigned gather_blocks(int64_t items) {
  const int64_t b = (items + GP_THREADS - 1) / GP_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > (int64_t)GP_MAX_BLOCKS ? (int64_t)GP_MAX_BLOCKS : b));
}

}  // namespace
