// gcs_index.h -- index plans of the PTv3 point backbone (gcs_serialize, gcs_patch_plan_*, include/gcs.h): the
// serialization codes of models/pt_v3.py's Point.serialization with their order and inverse, and the padding plan of
// SerializedAttention.get_padding_and_inverse.  Included by gcs_sparse.hip after its host helpers (align_up, fail);
// device code and launch helpers only, the C ABI stays in gcs_sparse.hip.  DESIGN.md section 15.5.
//
// Everything here is integer work on (grid_coord, batch) and (offset, patch_size); the only float expression is the
// `cord` code, three binary32 operations with IEEE division (the library's build flags: correctly rounded division,
// no contraction).  All kernels run on the caller's stream in caller-supplied workspace.
//   codes    k_index_codes: a thread per point computes every requested order's int64 code from one read of the row,
//            and the block adds the 8 byte-digit histograms of each order row to ghist (LDS, then integer atomics).
//   plan     k_index_plan: a block per order row marks a pass whose digit is constant over all keys (one bin of its
//            histogram holds n) as skipped, and gives every remaining pass its source and destination buffer, so that
//            the last one lands in the caller's `order` / `inverse`.  The host never learns which passes run: every
//            later kernel reads its pass's plan word and returns at once when the pass is skipped.
//   sort     stable LSD radix sort of (code, row), 8 bits a pass, the structure of gce_det.h's sort (per-block
//            histogram, scan per digit, ranked scatter) with 64-bit keys: the rows move, the keys stay in `code` and are
//            read through the row (the order rows of a frame fit the L2).  The sign bit is flipped in the digit of the
//            last pass: signed ascending.  Ties keep the lower row first (torch.sort(stable=True)).  All order rows sort
//            in the same launches (blockIdx.y).  The last pass that runs writes order[pos] = row and inverse[row] = pos.
//            Up to IX_SCAN_MIN_BLOCKS blocks of rows the scan is part of the scatter (two launches a pass, not three).
//   patch    k_patch_count (one block: padded rows and cu_seqlens entries, written to pinned host memory) and
//            k_patch_emit (blocks per batch: the batch's padded start is a sum over the batches before it).
#pragma once

namespace {

constexpr int IX_THREADS = 256;  // threads per block of every kernel here
constexpr int IX_ITEMS = 16;     // keys per thread
constexpr int IX_TILE = IX_THREADS * IX_ITEMS;
constexpr int IX_BITS = 8;
constexpr int IX_RADIX = 1 << IX_BITS;
constexpr int IX_PASSES = 8;   // 64-bit keys
constexpr uint32_t IX_SCAN_MIN_BLOCKS = 256;  // blocks (of IX_TILE rows) above which the per-block counts get a scan kernel
constexpr int IX_ORDERS = 5;   // enum gcs_order
constexpr uint64_t IX_SIGN = 1ull << 63;
// plan word of (order row, pass): bits 0-1 source (IX_IDENTITY: the row is its position), bits 2-3 destination, bit 4 runs
constexpr uint32_t IX_IDENTITY = 0, IX_BUF_A = 1, IX_BUF_B = 2, IX_FINAL = 3, IX_RUNS = 16;

struct IndexOrders {
  int32_t n, v[IX_ORDERS];
};

// ------------------------------------------------------------------------------------------- codes
// bit i of a 21-bit value to bit 3 i
__device__ __forceinline__ uint64_t ix_spread(uint32_t a) {
  uint64_t x = a & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__device__ __forceinline__ uint64_t ix_interleave(uint32_t x, uint32_t y, uint32_t z) {
  return ix_spread(x) << 2 | ix_spread(y) << 1 | ix_spread(z);
}
// Skilling's axes-to-transpose on three axes of `depth` bits, the Gray step, then the interleave with axis 0 most
// significant.  The Gray step runs on the interleaved word: bit k of the result is the XOR of the bits k and above.
__device__ __forceinline__ uint64_t ix_hilbert(uint32_t x, uint32_t y, uint32_t z, int depth) {
  uint32_t X[3] = {x, y, z};
  for (uint32_t Q = 1u << (depth - 1); Q > 1; Q >>= 1) {
    const uint32_t P = Q - 1;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (X[i] & Q) {
        X[0] ^= P;  // invert axis 0 below Q
      } else {
        const uint32_t t = (X[0] ^ X[i]) & P;  // exchange the low bits of axis 0 and axis i
        X[0] ^= t;
        X[i] ^= t;
      }
    }
  }
  uint64_t h = ix_interleave(X[0], X[1], X[2]);
  h ^= h >> 1;
  h ^= h >> 2;
  h ^= h >> 4;
  h ^= h >> 8;
  h ^= h >> 16;
  h ^= h >> 32;
  return h;
}

__global__ __launch_bounds__(IX_THREADS) void k_index_codes(const int32_t* __restrict__ coord,
                                                            const int64_t* __restrict__ batch, int64_t n, int depth,
                                                            float div_x, float div_y, const IndexOrders orders,
                                                            int64_t* __restrict__ code, uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[IX_ORDERS * IX_PASSES * IX_RADIX];
  const uint32_t tid = threadIdx.x;
  const int bins = orders.n * IX_PASSES * IX_RADIX;
  for (int b = tid; b < bins; b += IX_THREADS) h[b] = 0;
  __syncthreads();
  const uint32_t mask = (1u << depth) - 1u;
  const int64_t base = (int64_t)blockIdx.x * IX_TILE;
  for (int it = 0; it < IX_ITEMS; it++) {
    const int64_t i = base + (int64_t)it * IX_THREADS + tid;
    if (i >= n) break;
    const int32_t cx = coord[3 * i], cy = coord[3 * i + 1], cz = coord[3 * i + 2];
    const uint32_t x = (uint32_t)cx & mask, y = (uint32_t)cy & mask, z = (uint32_t)cz & mask;
    const int64_t high = batch ? (int64_t)((uint64_t)batch[i] << (3 * depth)) : 0;
    for (int o = 0; o < orders.n; o++) {
      int64_t c;
      switch (orders.v[o]) {
        case GCS_ORDER_CORD: c = (int64_t)truncf(((float)cx / div_x + (float)cy / div_y) + (float)cz); break;
        case GCS_ORDER_Z: c = (int64_t)ix_interleave(x, y, z); break;
        case GCS_ORDER_Z_TRANS: c = (int64_t)ix_interleave(y, x, z); break;
        case GCS_ORDER_HILBERT: c = (int64_t)ix_hilbert(x, y, z, depth); break;
        default: c = (int64_t)ix_hilbert(y, x, z, depth); break;
      }
      c |= high;
      code[(int64_t)o * n + i] = c;
      const uint64_t u = (uint64_t)c ^ IX_SIGN;
      uint32_t* ho = h + o * IX_PASSES * IX_RADIX;
#pragma unroll
      for (int p = 0; p < IX_PASSES; p++) atomicAdd(&ho[p * IX_RADIX + (uint32_t)(u >> (p * IX_BITS) & (IX_RADIX - 1))], 1u);
    }
  }
  __syncthreads();
  for (int b = tid; b < bins; b += IX_THREADS)
    if (h[b]) atomicAdd(&ghist[b], h[b]);
}

// ------------------------------------------------------------------------------------------- plan
__global__ __launch_bounds__(IX_THREADS) void k_index_plan(const uint32_t* __restrict__ ghist, uint32_t n,
                                                           uint32_t* __restrict__ plan) {
  __shared__ uint32_t constant[IX_PASSES];
  const uint32_t tid = threadIdx.x;
  if (tid < IX_PASSES) constant[tid] = 0;
  __syncthreads();
  const uint32_t* g = ghist + (size_t)blockIdx.x * IX_PASSES * IX_RADIX;
  for (int p = 0; p < IX_PASSES; p++)
    if (g[p * IX_RADIX + tid] == n) constant[p] = 1;  // at most one bin of a pass can hold all n keys
  __syncthreads();
  if (tid != 0) return;
  uint32_t runs = 0;
  for (int p = 0; p < IX_PASSES; p++)
    if (!constant[p]) runs |= 1u << p;
  if (!runs) runs = 1;  // all codes equal: pass 0 still runs and writes order = inverse = positions
  int k = 0;
  const int last = 31 - __clz(runs);
  for (int p = 0; p < IX_PASSES; p++) {
    uint32_t word = 0;
    if (runs >> p & 1u) {
      const uint32_t src = k == 0 ? IX_IDENTITY : ((k - 1) & 1 ? IX_BUF_B : IX_BUF_A);
      const uint32_t dst = p == last ? IX_FINAL : (k & 1 ? IX_BUF_B : IX_BUF_A);
      word = IX_RUNS | src | dst << 2;
      k++;
    }
    plan[blockIdx.x * IX_PASSES + p] = word;
  }
}

// ------------------------------------------------------------------------------------------- sort
struct IndexSort {
  uint32_t* rows[2];  // [orders][n] each: the rows in the order of the passes so far (IX_BUF_A, IX_BUF_B)
  uint32_t* table;    // [orders][IX_RADIX][nb] per-block digit counts of the running pass, scanned in place
  uint32_t* ghist;    // [orders][IX_PASSES][IX_RADIX] digit totals
  uint32_t* plan;     // [orders][IX_PASSES]
};

__device__ __forceinline__ uint32_t ix_digit(uint64_t key, int pass) {
  return (uint32_t)((key ^ IX_SIGN) >> (pass * IX_BITS)) & (IX_RADIX - 1);
}
// the key at position idx of the pass's source; a row outside [0, n) cannot come out of a consistent pass and reads row 0
__device__ __forceinline__ uint32_t ix_row(const uint32_t* __restrict__ src, uint32_t idx, uint32_t n) {
  if (!src) return idx;
  const uint32_t r = src[idx];
  return r < n ? r : 0u;
}
__device__ __forceinline__ const uint32_t* ix_source(const IndexSort& s, uint32_t word, uint32_t n) {
  const uint32_t c = word & 3u;
  return c == IX_IDENTITY ? nullptr : s.rows[c - 1] + (size_t)blockIdx.y * n;
}

__device__ __forceinline__ uint32_t ix_block_excl_scan(uint32_t v, uint32_t* lds4, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d);
    if (lane >= (uint32_t)d) inc += t;
  }
  if (lane == 63) lds4[w] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t c = lds4[k];
    if (k < w) base += c;
    tot += c;
  }
  __syncthreads();  // lds4 may be reused by the caller's next scan
  *total = tot;
  return base + inc - v;
}

// per-block digit histogram of the pass -> table[digit][block]; every entry is written, nothing is cleared first
__global__ __launch_bounds__(IX_THREADS) void k_index_radix_hist(const int64_t* __restrict__ code, uint32_t n, int pass,
                                                                 uint32_t nb, const IndexSort s) {
  const uint32_t word = s.plan[blockIdx.y * IX_PASSES + pass];
  if (!(word & IX_RUNS)) return;
  __shared__ uint32_t h[IX_RADIX];
  const uint32_t tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const uint32_t* src = ix_source(s, word, n);
  const int64_t* keys = code + (size_t)blockIdx.y * n;
  const uint32_t base = blockIdx.x * IX_TILE;
#pragma unroll 4
  for (int i = 0; i < IX_ITEMS; i++) {
    const uint32_t idx = base + i * IX_THREADS + tid;
    if (idx < n) atomicAdd(&h[ix_digit((uint64_t)keys[ix_row(src, idx, n)], pass)], 1u);
  }
  __syncthreads();
  s.table[((size_t)blockIdx.y * IX_RADIX + tid) * nb + blockIdx.x] = h[tid];
}

// one block per (digit, order row): exclusive scan of table[digit][0..nb) in place
__global__ __launch_bounds__(IX_THREADS) void k_index_radix_scan(int pass, uint32_t nb, const IndexSort s) {
  if (!(s.plan[blockIdx.y * IX_PASSES + pass] & IX_RUNS)) return;
  __shared__ uint32_t lds4[4];
  uint32_t* row = s.table + ((size_t)blockIdx.y * IX_RADIX + blockIdx.x) * nb;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += IX_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? row[i] : 0u;
    uint32_t total;
    const uint32_t ex = ix_block_excl_scan(v, lds4, &total);
    if (i < nb) row[i] = running + ex;
    running += total;
  }
}

// stable scatter of the rows by the pass's digit; the pass whose destination is IX_FINAL writes order and inverse
__global__ __launch_bounds__(IX_THREADS) void k_index_radix_scatter(const int64_t* __restrict__ code, uint32_t n, int pass,
                                                                    uint32_t nb, bool scanned, const IndexSort s,
                                                                    int64_t* __restrict__ order,
                                                                    int64_t* __restrict__ inverse) {
  const uint32_t word = s.plan[blockIdx.y * IX_PASSES + pass];
  if (!(word & IX_RUNS)) return;
  __shared__ uint32_t cnt[4][IX_RADIX];  // per-wave running digit counts
  __shared__ uint32_t dbase[IX_RADIX];   // output base of (digit, this block)
  __shared__ uint32_t lds4[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int i = 0; i < 4; i++) cnt[i][tid] = 0;
  {
    uint32_t total;
    const uint32_t gb = ix_block_excl_scan(s.ghist[((size_t)blockIdx.y * IX_PASSES + pass) * IX_RADIX + tid], lds4, &total);
    const uint32_t* counts = s.table + ((size_t)blockIdx.y * IX_RADIX + tid) * nb;
    uint32_t before = 0;  // keys with this digit in the blocks in front of this one
    if (scanned) {
      before = counts[blockIdx.x];
    } else {
      for (uint32_t b = 0; b < blockIdx.x; b++) before += counts[b];
    }
    dbase[tid] = gb + before;
  }
  __syncthreads();
  const uint32_t* src = ix_source(s, word, n);
  const int64_t* keys = code + (size_t)blockIdx.y * n;
  // wave w owns the contiguous slice [base + w * 1024, + 1024); element (i, lane) is base + w * 1024 + i * 64 + lane, so
  // (wave, i, lane) order is input order: stability
  const uint32_t wbase = blockIdx.x * IX_TILE + w * (64 * IX_ITEMS);
  uint32_t row[IX_ITEMS], lrank[IX_ITEMS];
  uint8_t dig[IX_ITEMS];
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < IX_ITEMS; i++) {
    const uint32_t idx = wbase + i * 64 + lane;
    const bool valid = idx < n;
    row[i] = valid ? ix_row(src, idx, n) : 0u;
    const uint32_t d = valid ? ix_digit((uint64_t)keys[row[i]], pass) : IX_RADIX - 1;
    dig[i] = (uint8_t)d;
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < IX_BITS; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bb = __ballot(bit);
      m &= bit ? bb : ~bb;
    }
    const uint32_t rank_in = (uint32_t)__popcll(m & lt_mask);
    const uint32_t old = cnt[w][d];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank_in == 0) cnt[w][d] = old + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
    lrank[i] = old + rank_in;
  }
  __syncthreads();
  {  // exclusive prefix of the per-wave counts across the four waves, per digit
    uint32_t run = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t t = cnt[i][tid];
      cnt[i][tid] = run;
      run += t;
    }
  }
  __syncthreads();
  const uint32_t dst = word >> 2 & 3u;
  uint32_t* out = dst == IX_FINAL ? nullptr : s.rows[dst - 1] + (size_t)blockIdx.y * n;
  int64_t* ord = order + (size_t)blockIdx.y * n;
  int64_t* inv = inverse + (size_t)blockIdx.y * n;
#pragma unroll
  for (int i = 0; i < IX_ITEMS; i++) {
    const uint32_t idx = wbase + i * 64 + lane;
    if (idx < n) {
      const uint32_t d = dig[i];
      const uint32_t pos = dbase[d] + cnt[w][d] + lrank[i];
      if (pos < n) {  // always true for a consistent histogram; keeps a broken one inside the buffers
        if (out) {
          out[pos] = row[i];
        } else {
          ord[pos] = (int64_t)row[i];
          inv[row[i]] = (int64_t)pos;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- workspace and launches
struct IndexLayout {
  uint32_t nb;
  size_t rows[2], table, ghist, plan, total;
};
inline IndexLayout index_layout(int64_t n, int32_t n_orders) {
  IndexLayout lay;
  lay.nb = (uint32_t)((n + IX_TILE - 1) / IX_TILE);
  size_t o = 0;
  for (int h = 0; h < 2; h++) { lay.rows[h] = o; o += align_up(sizeof(uint32_t) * (size_t)n * n_orders); }
  lay.table = o; o += align_up(sizeof(uint32_t) * (size_t)IX_RADIX * lay.nb * n_orders);
  lay.ghist = o; o += align_up(sizeof(uint32_t) * (size_t)IX_PASSES * IX_RADIX * n_orders);
  lay.plan = o;  o += align_up(sizeof(uint32_t) * (size_t)IX_PASSES * n_orders);
  lay.total = o;
  return lay;
}

// 0 < n < 2^31, orders checked
inline hipError_t index_serialize_launch(const int32_t* coord, const int64_t* batch, int64_t n, int depth, float div_x,
                                         float div_y, const IndexOrders& orders, int64_t* code, int64_t* order,
                                         int64_t* inverse, char* ws, hipStream_t st) {
  const IndexLayout lay = index_layout(n, orders.n);
  IndexSort s;
  s.rows[0] = (uint32_t*)(ws + lay.rows[0]);
  s.rows[1] = (uint32_t*)(ws + lay.rows[1]);
  s.table = (uint32_t*)(ws + lay.table);
  s.ghist = (uint32_t*)(ws + lay.ghist);
  s.plan = (uint32_t*)(ws + lay.plan);
  hipError_t e = hipMemsetAsync(s.ghist, 0, sizeof(uint32_t) * IX_PASSES * IX_RADIX * orders.n, st);
  if (e != hipSuccess) return e;
  k_index_codes<<<lay.nb, IX_THREADS, 0, st>>>(coord, batch, n, depth, div_x, div_y, orders, code, s.ghist);
  k_index_plan<<<orders.n, IX_THREADS, 0, st>>>(s.ghist, (uint32_t)n, s.plan);
  const dim3 tiles(lay.nb, orders.n), digits(IX_RADIX, orders.n);
  // Up to IX_SCAN_MIN_BLOCKS blocks (a frame's point set has 37 at most) a scatter block sums the counts of the blocks in
  // front of it itself, and a pass is two launches; beyond, that sum is a kernel of its own.
  const bool scanned = lay.nb > IX_SCAN_MIN_BLOCKS;
  for (int p = 0; p < IX_PASSES; p++) {
    k_index_radix_hist<<<tiles, IX_THREADS, 0, st>>>(code, (uint32_t)n, p, lay.nb, s);
    if (scanned) k_index_radix_scan<<<digits, IX_THREADS, 0, st>>>(p, lay.nb, s);
    k_index_radix_scatter<<<tiles, IX_THREADS, 0, st>>>(code, (uint32_t)n, p, lay.nb, scanned, s, order, inverse);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------- patch plan
// rows of batch i after padding: whole patches once the batch is longer than one patch
__device__ __forceinline__ int64_t ix_padded_rows(int64_t rows, int64_t P) { return rows > P ? (rows + P - 1) / P * P : rows; }
__device__ __forceinline__ int64_t ix_batch_rows(const int64_t* __restrict__ offset, int i) {
  const int64_t r = offset[i] - (i ? offset[i - 1] : 0);
  return r > 0 ? r : 0;
}
__device__ __forceinline__ int64_t ix_block_sum(int64_t v, int64_t* lds4) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  const int64_t t = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  __syncthreads();
  return t;
}

// one block: counts[0] = padded rows, counts[1] = cu_seqlens entries (the patches of every batch, and the total)
__global__ __launch_bounds__(IX_THREADS) void k_patch_count(const int64_t* __restrict__ offset, int nbatch, int64_t P,
                                                            int64_t* counts) {
  __shared__ int64_t lds4[4];
  int64_t rows = 0, cu = 0;
  for (int i = threadIdx.x; i < nbatch; i += IX_THREADS) {
    const int64_t np = ix_padded_rows(ix_batch_rows(offset, i), P);
    rows += np;
    cu += (np + P - 1) / P;
  }
  rows = ix_block_sum(rows, lds4);
  cu = ix_block_sum(cu, lds4);
  if (threadIdx.x == 0) {
    counts[0] = rows;
    counts[1] = cu + 1;
    __threadfence_system();
  }
}

// blockIdx.x = batch, blockIdx.y = a slice of its rows.  Every store is held inside the arrays' lengths, so offsets that
// changed after gcs_patch_plan_count leave a wrong plan, not a stray write.
__global__ __launch_bounds__(IX_THREADS) void k_patch_emit(const int64_t* __restrict__ offset, int nbatch, int64_t P,
                                                           int64_t padded, int64_t n_cu, int64_t* __restrict__ pad,
                                                           int64_t* __restrict__ unpad, int32_t* __restrict__ cu_seqlens) {
  __shared__ int64_t lds4[4];
  const int b = blockIdx.x;
  int64_t before = 0, cu_before = 0;  // padded rows and cu_seqlens entries of the batches in front of this one
  for (int i = threadIdx.x; i < b; i += IX_THREADS) {
    const int64_t np = ix_padded_rows(ix_batch_rows(offset, i), P);
    before += np;
    cu_before += (np + P - 1) / P;
  }
  before = ix_block_sum(before, lds4);
  cu_before = ix_block_sum(cu_before, lds4);
  const int64_t rows = ix_batch_rows(offset, b), np = ix_padded_rows(rows, P);
  const int64_t start = b ? offset[b - 1] : 0, shift = before - start, total = offset[nbatch - 1];
  const int64_t first = (int64_t)blockIdx.y * IX_THREADS + threadIdx.x, step = (int64_t)gridDim.y * IX_THREADS;
  for (int64_t r = first; r < np; r += step) {
    const int64_t p = before + r;
    if (p < padded) pad[p] = (r >= rows ? p - P : p) - shift;  // the padded tail repeats the rows one patch before it
    if (r < rows && start + r < total) unpad[start + r] = p;
  }
  const int64_t patches = (np + P - 1) / P;
  for (int64_t m = first; m < patches; m += step)
    if (cu_before + m < n_cu) cu_seqlens[cu_before + m] = (int32_t)(before + m * P);
  if (b == nbatch - 1 && first == 0 && cu_before + patches < n_cu) cu_seqlens[cu_before + patches] = (int32_t)(before + np);
}

}  // namespace
