// gce_det.h -- deterministic table gradient of the hash-grid encoder (gce_backward_det, include/gce.h): no float
// atomics, every table row summed in one fixed order.  Included by gce_grid.hip after its device helpers (locate,
// grid_index, GceOps, LevelScales); device code and launch helpers only, the C ABI stays in gce_grid.hip.
//
// n = L * B * 2^D contributions, contribution id = (level * B + point) * 2^D + corner (the order in which k_grid_bwd
// enumerates them).  Three steps, all on the caller's stream, all in caller-supplied workspace:
//   keys     k_det_keys: key[id] = global table row of the contribution (offsets[level] + row), or the sentinel
//            total_rows for a point outside [0,1] / a row past the table.  The sentinel sorts last and is never stored.
//   sort     stable LSD radix sort of (key, id) on the bits total_rows needs, 8 bits a pass (hist / scan / scatter, the
//            pattern of gcr_binning.hip's K4 for u32 keys; the first pass makes up id = position instead of reading it).
//            Stable + id-ordered input: every row's contributions are consecutive, in ascending id.
//   reduce   k_det_reduce over fixed tiles of DET_TILE = 256 sorted entries, one entry per thread: the thread recomputes
//            its term from id (same w * gc product and rounding as the atomic kernels), a segmented scan by key over the
//            wave (6 shuffle steps) and over the workgroup's 4 waves (3 steps) sums every run of equal keys in an order
//            that depends on the positions alone.  A run that neither began in the previous tile nor goes on in the next
//            has one owner: table[row] = old + sum, a plain store.  A run that crosses a tile edge leaves a record (key,
//            sum) in one of the tile's two slots; the records of all tiles, in tile order, are again a sequence in which
//            equal keys are consecutive, so the same kernel reduces them (LEAF = false), and again, until one tile holds
//            what is left: n -> 2 * ceil(n / 256) -> ... (4 levels for n = 8.4 M, 5 below 2^31).  No thread's serial
//            work depends on the length of a run.
// Every slot of every level is written before it is read, so what the workspace held before does not matter.
#pragma once

namespace {

constexpr int DET_TILE = 256;         // entries per reduce workgroup (one per thread)
constexpr int RS_THREADS = 256;       // radix sort: threads per block
constexpr int RS_ITEMS = 16;          // keys per thread
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;
constexpr int RS_BITS = 8;
constexpr int RS_RADIX = 1 << RS_BITS;
constexpr int DET_MAX_LEVELS = 8;     // reduce levels; 5 suffice below n = 2^31

template <typename T>
struct DetAcc {
  typedef float type;  // float and binary16 tables sum in float
};
template <>
struct DetAcc<double> {
  typedef double type;
};

// ------------------------------------------------------------------------------------------- keys
// thread = (point, level), as k_grid_fwd: the 2^D keys of one (level, point) are consecutive ids
template <int D>
__global__ __launch_bounds__(256) void k_det_keys(const float* __restrict__ inputs, const int32_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ keys, uint32_t total_rows, uint32_t B,
                                                  const LevelScales scales, uint32_t gridtype, bool align_corners) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint32_t level = blockIdx.y;
  const uint32_t off0 = (uint32_t)offsets[level], off1 = (uint32_t)offsets[level + 1];
  uint32_t* __restrict__ out = keys + (((size_t)level * B + b) << D);
  const float scale = scales.v[level];
  const uint32_t hashmap_size = off1 - off0;
  float pos[D];
  uint32_t pos_grid[D];
  if (hashmap_size == 0 || !locate<D>(inputs + (size_t)b * D, scale, align_corners, pos, pos_grid)) {
#pragma unroll
    for (uint32_t idx = 0; idx < (1u << D); idx++) out[idx] = total_rows;
    return;
  }
  const uint32_t resolution = (uint32_t)ceil(scale) + 1;
#pragma unroll
  for (uint32_t idx = 0; idx < (1u << D); idx++) {
    uint32_t pl[D];
#pragma unroll
    for (int d = 0; d < D; d++) pl[d] = pos_grid[d] + ((idx >> d) & 1u);
    const uint64_t row = (uint64_t)off0 + grid_index<D, 1>(gridtype, align_corners, hashmap_size, resolution, pl);
    out[idx] = row < total_rows ? (uint32_t)row : total_rows;
  }
}

// ------------------------------------------------------------------------------------------- sort
__device__ __forceinline__ uint32_t det_block_excl_scan_256(uint32_t v, uint32_t* lds4, uint32_t* total) {
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

// per-block digit histogram -> table[digit][block], and the digit totals of the pass
__global__ __launch_bounds__(RS_THREADS) void k_det_radix_hist(const uint32_t* __restrict__ keys, uint32_t n, int shift,
                                                               uint32_t nb, uint32_t* __restrict__ table,
                                                               uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[RS_RADIX];
  const uint32_t tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * RS_TILE;
#pragma unroll 4
  for (int i = 0; i < RS_ITEMS; i++) {
    const uint32_t idx = base + i * RS_THREADS + tid;
    if (idx < n) atomicAdd(&h[(keys[idx] >> shift) & (RS_RADIX - 1)], 1u);
  }
  __syncthreads();
  const uint32_t c = h[tid];
  table[(size_t)tid * nb + blockIdx.x] = c;
  if (c) atomicAdd(&ghist[tid], c);
}

// one block per digit: exclusive scan of table[digit][0..nb) in place
__global__ __launch_bounds__(256) void k_det_radix_scan(uint32_t* __restrict__ table, uint32_t nb) {
  __shared__ uint32_t lds4[4];
  uint32_t* row = table + (size_t)blockIdx.x * nb;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < nb ? row[i] : 0u;
    uint32_t total;
    const uint32_t ex = det_block_excl_scan_256(v, lds4, &total);
    if (i < nb) row[i] = running + ex;
    running += total;
  }
}

// stable scatter; vin == nullptr stands for the identity (first pass: id = position)
__global__ __launch_bounds__(RS_THREADS) void k_det_radix_scatter(const uint32_t* __restrict__ kin,
                                                                  const uint32_t* __restrict__ vin,
                                                                  uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                                  uint32_t n, int shift, uint32_t nb,
                                                                  const uint32_t* __restrict__ table,
                                                                  const uint32_t* __restrict__ ghist) {
  __shared__ uint32_t cnt[4][RS_RADIX];  // per-wave running digit counts
  __shared__ uint32_t dbase[RS_RADIX];   // global output base of (digit, this block)
  __shared__ uint32_t lds4[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int i = 0; i < 4; i++) cnt[i][tid] = 0;
  {
    uint32_t total;
    const uint32_t gb = det_block_excl_scan_256(ghist[tid], lds4, &total);
    dbase[tid] = gb + table[(size_t)tid * nb + blockIdx.x];
  }
  __syncthreads();
  // wave w owns the contiguous slice [base + w * 1024, + 1024); element (i, lane) is base + w * 1024 + i * 64 + lane, so
  // (wave, i, lane) order is input order: stability
  const uint32_t wbase = blockIdx.x * RS_TILE + w * (64 * RS_ITEMS);
  uint32_t key[RS_ITEMS], lrank[RS_ITEMS];
  const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < RS_ITEMS; i++) {
    const uint32_t idx = wbase + i * 64 + lane;
    const bool valid = idx < n;
    key[i] = valid ? kin[idx] : ~0u;
    const uint32_t d = (key[i] >> shift) & (RS_RADIX - 1);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RS_BITS; b++) {
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
#pragma unroll
  for (int i = 0; i < RS_ITEMS; i++) {
    const uint32_t idx = wbase + i * 64 + lane;
    if (idx < n) {
      const uint32_t d = (key[i] >> shift) & (RS_RADIX - 1);
      const uint32_t pos = dbase[d] + cnt[w][d] + lrank[i];
      if (pos < n) {  // always true for a consistent histogram; keeps a broken one inside the buffers
        kout[pos] = key[i];
        vout[pos] = vin ? vin[idx] : idx;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- reduce
// The element of the scan: a sum that may be absent.  Level 0 entries always carry one; a record slot of a higher level
// may be empty (a tile has two slots and fills the ones it needs).  a (+) b keeps the order "earlier + later".
template <typename A, int C>
struct DetVal {
  A v[C];
  bool has;
};
template <typename A, int C>
__device__ __forceinline__ void det_combine_left(const DetVal<A, C>& left, DetVal<A, C>& x) {  // x = left (+) x
  if (!left.has) return;
#pragma unroll
  for (int ch = 0; ch < C; ch++) x.v[ch] = x.has ? left.v[ch] + x.v[ch] : left.v[ch];
  x.has = true;
}

// keys / src: the level's entries.  LEAF: src = sorted contribution ids, the term is recomputed.  Otherwise src = the
// records' "has a sum" flags and in_sum their sums.  out_*: the next level's records, two slots per tile (null on the
// last level, which is one tile and leaves none).
template <typename T, int D, int C, bool LEAF>
__global__ __launch_bounds__(DET_TILE) void k_det_reduce(
    const uint32_t* __restrict__ keys, const uint32_t* __restrict__ src, const typename DetAcc<T>::type* __restrict__ in_sum,
    uint32_t count, const T* __restrict__ grad, const float* __restrict__ inputs, T* __restrict__ grad_grid,
    uint32_t total_rows, uint32_t B, const LevelScales scales, bool align_corners, uint32_t* __restrict__ out_key,
    uint32_t* __restrict__ out_has, typename DetAcc<T>::type* __restrict__ out_sum) {
  using A = typename DetAcc<T>::type;
  __shared__ float s_scale[GCE_MAX_LEVELS];
  __shared__ uint32_t s_key_first[4], s_key_last[4], s_single[4], s_agg_has[4];
  __shared__ A s_agg[4][C];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t i = blockIdx.x * DET_TILE + tid;
  const bool in = i < count;
  if constexpr (LEAF) {
#pragma unroll
    for (uint32_t l = 0; l < GCE_MAX_LEVELS; l++)
      if (tid == l) s_scale[l] = scales.v[l];
    __syncthreads();
  }
  const uint32_t key = in ? keys[i] : total_rows;  // the padding of the last tile joins the sentinel run
  constexpr uint32_t NO_KEY = 0xFFFFFFFFu;         // total_rows <= 2^31 - 1: never a key
  const uint32_t next_key = (in && i + 1 < count) ? keys[i + 1] : NO_KEY;

  DetVal<A, C> x;
  x.has = false;
#pragma unroll
  for (int ch = 0; ch < C; ch++) x.v[ch] = (A)0;
  if (in && key < total_rows) {
    if constexpr (LEAF) {
      const uint32_t id = src[i];
      const uint32_t corner = id & ((1u << D) - 1u), lb = id >> D;
      const uint32_t level = lb / B, b = lb - level * B;
      float pos[D];
      uint32_t pos_grid[D];
      if (id < count && level < GCE_MAX_LEVELS && locate<D>(inputs + (size_t)b * D, s_scale[level], align_corners, pos, pos_grid)) {
        float w = 1;  // the same products, in the same order, as k_grid_bwd / k_grid_bwd_t
#pragma unroll
        for (int d = 0; d < D; d++) {
          if ((corner & (1u << d)) == 0) {
            w *= 1 - pos[d];
          } else {
            w *= pos[d];
          }
        }
        const T* __restrict__ g = grad + ((size_t)level * B + b) * C;
#pragma unroll
        for (int ch = 0; ch < C; ch++) x.v[ch] = (A)GceOps<T>::mulw(w, g[ch]);
        x.has = true;
      }
    } else {
      if (src[i]) {
#pragma unroll
        for (int ch = 0; ch < C; ch++) x.v[ch] = in_sum[(size_t)i * C + ch];
        x.has = true;
      }
    }
  }

  // segmented inclusive scan over the wave: a run of equal keys is a segment
  const uint32_t prev_key = __shfl_up(key, 1);
  const bool head = lane == 0 || prev_key != key;
  const uint64_t heads = __ballot(head);
  const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const int seg0 = 63 - __clzll((long long)(heads & upto));  // first lane of this lane's segment (bit 0 is always set)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int from = (int)lane - d;
    DetVal<A, C> o;
    o.has = __shfl((int)x.has, from & 63) != 0;
#pragma unroll
    for (int ch = 0; ch < C; ch++) o.v[ch] = __shfl(x.v[ch], from & 63);
    if (from < seg0) o.has = false;
    det_combine_left(o, x);
  }

  // across the four waves: R = the sum of the run that ends with the previous wave's last lane
  if (lane == 0) s_key_first[wv] = key;
  if (lane == 63) {
    s_key_last[wv] = key;
    s_single[wv] = seg0 == 0;
    s_agg_has[wv] = x.has;
#pragma unroll
    for (int ch = 0; ch < C; ch++) s_agg[wv][ch] = x.v[ch];
  }
  __syncthreads();
  DetVal<A, C> R;
  R.has = false;
#pragma unroll
  for (int ch = 0; ch < C; ch++) R.v[ch] = (A)0;
  bool r_from0 = false;  // that run began at the tile's first entry
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    if (k < wv) {
      DetVal<A, C> a;
      a.has = s_agg_has[k] != 0;
#pragma unroll
      for (int ch = 0; ch < C; ch++) a.v[ch] = s_agg[k][ch];
      const bool cont = k > 0 && s_single[k] && s_key_last[k - 1] == s_key_first[k];
      if (cont) {
        det_combine_left(R, a);
      } else {
        r_from0 = k == 0 && s_single[0];
      }
      R = a;
    }
  }
  bool from0 = wv == 0 && seg0 == 0;  // this lane's run began at the tile's first entry
  if (wv > 0 && seg0 == 0 && s_key_last[wv - 1] == key) {
    det_combine_left(R, x);
    from0 = r_from0;
  }

  if (!in) return;
  const bool tile_last = tid == DET_TILE - 1 || i + 1 == count;
  const bool run_end = tile_last || next_key != key;
  if (!run_end) return;
  const bool row = key < total_rows;
  const bool open_right = next_key == key;  // only a tile's last entry gets here with it
  const bool open_left = from0 && blockIdx.x > 0 && keys[(size_t)blockIdx.x * DET_TILE - 1] == key;
  const bool open = row && (open_left || open_right);
  if (row && !open && x.has) {  // the run's one owner: old + sum, rounded once
    T* __restrict__ dst = grad_grid + (size_t)key * C;
#pragma unroll
    for (int ch = 0; ch < C; ch++) dst[ch] = (T)((A)dst[ch] + x.v[ch]);
  }
  if (!out_key) return;
  const size_t slot0 = (size_t)blockIdx.x * 2;
  if (open) {
    const size_t slot = slot0 + (from0 ? 0 : 1);
    out_key[slot] = key;
    out_has[slot] = x.has;
#pragma unroll
    for (int ch = 0; ch < C; ch++) out_sum[slot * C + ch] = x.v[ch];
  } else if (from0) {
    out_key[slot0] = total_rows;
    out_has[slot0] = 0;
  }
  if (tile_last && !(open && !from0)) {
    // second slot unused.  After a run that fills the whole tile it keeps the run's key, so that the run's records in
    // the neighbouring tiles stay consecutive
    out_key[slot0 + 1] = (from0 && open) ? key : total_rows;
    out_has[slot0 + 1] = 0;
  }
}

// ------------------------------------------------------------------------------------------- workspace and launches
struct DetLayout {
  uint32_t n, nb, passes, levels;
  uint32_t level_count[DET_MAX_LEVELS];  // entries of reduce level k (level 0: n)
  size_t level_base[DET_MAX_LEVELS];     // first record of level k >= 1 in the record arrays
  size_t keys[2], ids[2], table, ghist, rec_key, rec_has, rec_sum, total;
};

inline size_t det_align(size_t x) { return (x + 255) & ~(size_t)255; }

// n < 2^31, n > 0
inline DetLayout det_layout(uint32_t n, uint32_t total_rows) {
  DetLayout lay;
  lay.n = n;
  lay.nb = (n + RS_TILE - 1) / RS_TILE;
  uint32_t bits = 0;
  while (bits < 32 && (total_rows >> bits)) bits++;  // the sentinel total_rows is the largest key
  lay.passes = bits ? (bits + RS_BITS - 1) / RS_BITS : 1;
  lay.levels = 0;
  size_t records = 0;
  for (uint32_t c = n;; c = 2 * ((c + DET_TILE - 1) / DET_TILE)) {
    lay.level_count[lay.levels] = c;
    lay.level_base[lay.levels] = lay.levels ? records : 0;
    if (lay.levels) records += c;
    lay.levels++;
    if (c <= (uint32_t)DET_TILE || lay.levels == DET_MAX_LEVELS) break;
  }
  size_t o = 0;
  for (int h = 0; h < 2; h++) { lay.keys[h] = o; o += det_align(sizeof(uint32_t) * (size_t)n); }
  for (int h = 0; h < 2; h++) { lay.ids[h] = o; o += det_align(sizeof(uint32_t) * (size_t)n); }
  lay.table = o;   o += det_align(sizeof(uint32_t) * (size_t)RS_RADIX * lay.nb);
  lay.ghist = o;   o += det_align(sizeof(uint32_t) * (size_t)RS_RADIX * 4);
  lay.rec_key = o; o += det_align(sizeof(uint32_t) * records);
  lay.rec_has = o; o += det_align(sizeof(uint32_t) * records);
  lay.rec_sum = o; o += det_align(sizeof(double) * 8 * records);  // the widest case: 8 channels of double
  lay.total = o;
  return lay;
}

template <typename T, int D, int C>
hipError_t det_launch(const T* grad, const float* inputs, const int32_t* offsets, T* grad_grid, uint32_t total_rows,
                      uint32_t B, uint32_t L, const LevelScales& sc, uint32_t gridtype, bool align_corners, char* ws,
                      const DetLayout& lay, hipStream_t s) {
  using A = typename DetAcc<T>::type;
  const uint32_t n = lay.n;
  uint32_t* kin = (uint32_t*)(ws + lay.keys[0]);
  uint32_t* kout = (uint32_t*)(ws + lay.keys[1]);
  uint32_t* vin = nullptr;  // first pass: id = position
  uint32_t* vout = (uint32_t*)(ws + lay.ids[0]);
  uint32_t* vnext = (uint32_t*)(ws + lay.ids[1]);
  uint32_t* table = (uint32_t*)(ws + lay.table);
  uint32_t* ghist = (uint32_t*)(ws + lay.ghist);
  k_det_keys<D><<<dim3((B + 255) / 256, L, 1), 256, 0, s>>>(inputs, offsets, kin, total_rows, B, sc, gridtype, align_corners);
  hipError_t e = hipMemsetAsync(ghist, 0, sizeof(uint32_t) * RS_RADIX * lay.passes, s);
  if (e != hipSuccess) return e;
  for (uint32_t p = 0; p < lay.passes; p++) {
    const int shift = (int)(p * RS_BITS);
    uint32_t* gh = ghist + (size_t)p * RS_RADIX;
    k_det_radix_hist<<<lay.nb, RS_THREADS, 0, s>>>(kin, n, shift, lay.nb, table, gh);
    k_det_radix_scan<<<RS_RADIX, 256, 0, s>>>(table, lay.nb);
    k_det_radix_scatter<<<lay.nb, RS_THREADS, 0, s>>>(kin, vin, kout, vout, n, shift, lay.nb, table, gh);
    uint32_t* t = kin; kin = kout; kout = t;
    vin = vout; vout = vnext; vnext = vin;
  }
  uint32_t* rec_key = (uint32_t*)(ws + lay.rec_key);
  uint32_t* rec_has = (uint32_t*)(ws + lay.rec_has);
  A* rec_sum = (A*)(ws + lay.rec_sum);
  for (uint32_t k = 0; k < lay.levels; k++) {
    const uint32_t count = lay.level_count[k];
    const uint32_t tiles = (count + DET_TILE - 1) / DET_TILE;
    const bool last = k + 1 == lay.levels;
    const size_t ob = last ? 0 : lay.level_base[k + 1];
    uint32_t* ok = last ? nullptr : rec_key + ob;
    uint32_t* oh = last ? nullptr : rec_has + ob;
    A* os = last ? nullptr : rec_sum + ob * C;
    if (k == 0) {
      k_det_reduce<T, D, C, true><<<tiles, DET_TILE, 0, s>>>(kin, vin, nullptr, count, grad, inputs, grad_grid, total_rows, B,
                                                           sc, align_corners, ok, oh, os);
    } else {
      const size_t ib = lay.level_base[k];
      k_det_reduce<T, D, C, false><<<tiles, DET_TILE, 0, s>>>(rec_key + ib, rec_has + ib, rec_sum + ib * C, count, grad, inputs,
                                                            grad_grid, total_rows, B, sc, align_corners, ok, oh, os);
    }
  }
  return hipGetLastError();
}

}  // namespace
