// gcv_split.h -- K17 (visible point set -> per-model generator inputs) and K18 ([N][14] Gaussians in one launch) of
// libgcv_hip.so; included by gcv_points.hip, whose helpers (fail, HIP_TRY, misaligned, vs_block_excl_scan) it uses.
// Reference behaviour: scripts/inference.py:239-253 with :399-507 (_get_z, _get_pt_indexes_by_models,
// _get_pt_attrs_by_models), utils/helpers.py:127-133 (get_one_hot), :183-194 (get_projection_uv), :226-247
// (get_gaussian_points).
//
// K17 is K16's shape once more -- count / scan / emit over a caller's workspace:
//   count  one thread per visible row: the row's model from its class (a 2-bit code per class in one 64-bit word), the
//          block's rows per model (wave ballots -> LDS -> three sums per block), and an atomic OR of the row's instance
//          rank into its model's K-bit presence table (a lane whose left neighbour holds the same model and rank leaves
//          the bit to it: visible rows of one instance are neighbours);
//   scan   one 1024-thread block: per model the block sums -> output offsets (model 0's rows first) and n_m; per presence
//          word the bits whose instance has a style code; per model the rank of each word's first instance among the
//          model's instances (B_m) and among those with a code (G_m);
//   emit   the count kernel's blocks again: a row's slot = its block's offset for the model + the ballots in front of it,
//          which is the order of a boolean-mask gather without a sort; the row is read once and every output written
//          from it; a second small kernel writes the per-model code tables.
// Integer work except proj_uv, which is three fp32 operations in upstream's order (IEEE division, no contraction).
// No float atomics; the only order-free operations are the bit ORs and the bad-row counter.
#pragma once

namespace {

constexpr int MS_BLOCK = 256;
constexpr int MS_MODELS = 3;
constexpr long long MS_MAX_INSTANCES = 65536;  // distinct int16 values
enum { MS_HEAD_N = 0, MS_HEAD_B = 3, MS_HEAD_G = 6, MS_HEAD_BAD = 9, MS_HEAD_WORDS = 16 };

// workspace: [head u32 x 16][presence u32 x 3 x n_words] -- cleared by every count -- then [has u32 x n_words]
// [rank_b u32 x 3 x n_words][rank_g u32 x 3 x n_words][block sums / offsets u32 x 3 x n_blocks]
struct SplitLayout {
  size_t presence, has, rank_b, rank_g, sums, total;
  int n_words;         // presence words per model
  long long n_blocks;  // blocks of the count / emit kernels
};
SplitLayout split_layout(long long m, long long k) {
  SplitLayout l;
  l.n_words = (int)((k + 31) / 32);
  l.n_blocks = (m + MS_BLOCK - 1) / MS_BLOCK;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  const size_t words = sizeof(uint32_t) * (size_t)l.n_words;
  l.presence = up(sizeof(uint32_t) * MS_HEAD_WORDS);
  l.has = l.presence + MS_MODELS * words;
  l.rank_b = l.has + words;
  l.rank_g = l.rank_b + MS_MODELS * words;
  l.sums = up(l.rank_g + MS_MODELS * words);
  l.total = up(l.sums + sizeof(uint32_t) * MS_MODELS * (size_t)(l.n_blocks + 1));
  return l;
}

struct SplitRule {
  int n_classes;
  unsigned long long model_bits;  // 2 bits per class: the model slot, 3 = dropped
  float tlp_x, tlp_y, size;
};

// The model of a row, -1 when it is dropped or bad.  *ci: its class as an integer.  *bad: the class is not an integer in
// [0, n_classes) or the rank is outside [0, K) -- such a row is dropped and indexes nothing.
__device__ __forceinline__ int split_model(const SplitRule& r, float c, int b, long long K, int* ci, bool* bad) {
  int cls = -1;
  if (c >= 0.0f && c < (float)r.n_classes) {  // (a NaN fails both)
    cls = (int)c;
    if ((float)cls != c) cls = -1;
  }
  *ci = cls;
  *bad = cls < 0 || b < 0 || (long long)b >= K;
  if (*bad) return -1;
  const int m = (int)((r.model_bits >> (2 * cls)) & 3ull);
  return m == 3 ? -1 : m;
}

// per-model ballots of the block: s_cnt[wave][model] = the wave's rows of that model; returns this lane's rank among its
// wave's rows of its own model (0 for a dropped row).  Ends with a barrier.
__device__ __forceinline__ uint32_t split_ballots(int model, uint32_t (*s_cnt)[MS_MODELS]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t rank = 0;
#pragma unroll
  for (int m = 0; m < MS_MODELS; m++) {
    const unsigned long long mask = __ballot(model == m);
    if (lane == 0) s_cnt[w][m] = (uint32_t)__popcll(mask);
    if (model == m) rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  return rank;
}

__global__ __launch_bounds__(MS_BLOCK) void k_split_count(const float* __restrict__ classes,
                                                          const int32_t* __restrict__ batch_index, long long M,
                                                          long long K, const SplitRule r, uint32_t* __restrict__ presence,
                                                          int n_words, uint32_t* __restrict__ sums,
                                                          uint32_t* __restrict__ head) {
  __shared__ uint32_t s_cnt[MS_BLOCK / 64][MS_MODELS];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * MS_BLOCK + tid;
  int model = -1, b = -1, ci;
  bool bad = false;
  if (i < M) {
    b = batch_index[i];
    model = split_model(r, classes[i], b, K, &ci, &bad);
  }
  if (bad) atomicAdd(&head[MS_HEAD_BAD], 1u);
  const int key = model >= 0 ? (model << 16) | b : -1;  // b < K <= 65536
  const int left = __shfl_up(key, 1, 64);
  if (model >= 0 && ((tid & 63) == 0 || left != key))
    atomicOr(&presence[(size_t)model * n_words + (b >> 5)], 1u << (b & 31));
  split_ballots(model, s_cnt);
  if (tid < MS_MODELS) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < MS_BLOCK / 64; w++) s += s_cnt[w][tid];
    sums[(size_t)blockIdx.x * MS_MODELS + tid] = s;
  }
}

// block sums -> output offsets in place (model 0's rows first) and n_m; presence words -> the bits that have a code, the
// rank of each word's first instance per model (all: rank_b, with a code: rank_g), B_m and G_m
__global__ __launch_bounds__(1024) void k_split_scan(uint32_t* __restrict__ sums, long long n_blocks,
                                                     const uint32_t* __restrict__ presence, int n_words,
                                                     const int16_t* __restrict__ instances, long long K,
                                                     const uint8_t* __restrict__ lut_has, int n_lut,
                                                     uint32_t* __restrict__ has, uint32_t* __restrict__ rank_b,
                                                     uint32_t* __restrict__ rank_g, uint32_t* __restrict__ head) {
  __shared__ uint32_t lds16[16];
  const int tid = threadIdx.x;
  const long long per = (n_blocks + 1023) / 1024;
  const long long beg = min(n_blocks, tid * per), end = min(n_blocks, beg + per);
  uint32_t base = 0;
  for (int m = 0; m < MS_MODELS; m++) {
    uint32_t s = 0, total;
    for (long long i = beg; i < end; i++) s += sums[i * MS_MODELS + m];
    uint32_t run = base + vs_block_excl_scan<16>(s, lds16, &total);
    for (long long i = beg; i < end; i++) {
      const uint32_t t = sums[i * MS_MODELS + m];
      sums[i * MS_MODELS + m] = run;
      run += t;
    }
    if (tid == 0) head[MS_HEAD_N + m] = total;
    base += total;
  }
  // two presence words per thread: n_words <= 2048
  uint32_t p[2][MS_MODELS], h[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int w = 2 * tid + j;
    uint32_t any = 0;
#pragma unroll
    for (int m = 0; m < MS_MODELS; m++) {
      p[j][m] = w < n_words ? presence[(size_t)m * n_words + w] : 0u;
      any |= p[j][m];
    }
    h[j] = 0u;
    while (any) {
      const int bit = __ffs((int)any) - 1;
      any &= any - 1;
      const long long rk = (long long)w * 32 + bit;
      if (rk >= K) continue;  // (the count kernel sets no such bit)
      const int id = instances[rk];
      if (id >= 0 && id < n_lut && lut_has[id] != 0) h[j] |= 1u << bit;
    }
    if (w < n_words) has[w] = h[j];
  }
  for (int m = 0; m < MS_MODELS; m++) {
    uint32_t total;
    uint32_t c0 = (uint32_t)__popc(p[0][m]), c1 = (uint32_t)__popc(p[1][m]);
    uint32_t rk = vs_block_excl_scan<16>(c0 + c1, lds16, &total);
    if (2 * tid < n_words) rank_b[(size_t)m * n_words + 2 * tid] = rk;
    if (2 * tid + 1 < n_words) rank_b[(size_t)m * n_words + 2 * tid + 1] = rk + c0;
    if (tid == 0) head[MS_HEAD_B + m] = total;
    c0 = (uint32_t)__popc(p[0][m] & h[0]);
    c1 = (uint32_t)__popc(p[1][m] & h[1]);
    rk = vs_block_excl_scan<16>(c0 + c1, lds16, &total);
    if (2 * tid < n_words) rank_g[(size_t)m * n_words + 2 * tid] = rk;
    if (2 * tid + 1 < n_words) rank_g[(size_t)m * n_words + 2 * tid + 1] = rk + c0;
    if (tid == 0) head[MS_HEAD_G + m] = total;
  }
}

struct SplitEmitArgs {
  const float *classes, *points8, *scales3;
  const int32_t* batch_index;
  long long M, K, N;
  SplitRule r;
  const uint32_t *presence, *has, *rank_b, *rank_g, *sums;
  int n_words;
  long long* index;
  float *points8_out, *classes_out, *scales3_out, *onehots, *proj_uv;
  int32_t *batch, *group;
};

__global__ __launch_bounds__(MS_BLOCK) void k_split_emit(const SplitEmitArgs a) {
  __shared__ uint32_t s_cnt[MS_BLOCK / 64][MS_MODELS];
  const int tid = threadIdx.x, wv = tid >> 6;
  const long long i = (long long)blockIdx.x * MS_BLOCK + tid;
  int model = -1, b = -1, ci = -1;
  bool bad = false;
  float c = 0.0f;
  if (i < a.M) {
    b = a.batch_index[i];
    c = a.classes[i];
    model = split_model(a.r, c, b, a.K, &ci, &bad);
  }
  const uint32_t rank = split_ballots(model, s_cnt);
  if (model < 0) return;
  long long o = (long long)a.sums[(size_t)blockIdx.x * MS_MODELS + model] + rank;
  for (int k = 0; k < wv; k++) o += s_cnt[k][model];
  if (o >= a.N) return;  // a stale workspace or count stays in bounds
  if (a.index != nullptr) a.index[o] = i;
  if (a.points8_out != nullptr || a.proj_uv != nullptr) {
    const float4* src = reinterpret_cast<const float4*>(a.points8 + 8 * i);
    const float4 lo = src[0];
    if (a.points8_out != nullptr) {
      float4* dst = reinterpret_cast<float4*>(a.points8_out + 8 * o);
      dst[0] = lo;
      dst[1] = src[1];
    }
    if (a.proj_uv != nullptr) {  // utils/helpers.py:188-194: subtract, divide, times 2, minus 1
      a.proj_uv[2 * o] = ((lo.x - a.r.tlp_x) / a.r.size) * 2.0f - 1.0f;
      a.proj_uv[2 * o + 1] = ((lo.y - a.r.tlp_y) / a.r.size) * 2.0f - 1.0f;
    }
  }
  if (a.classes_out != nullptr) a.classes_out[o] = c;
  if (a.scales3_out != nullptr) {
#pragma unroll
    for (int k = 0; k < 3; k++) a.scales3_out[3 * o + k] = a.scales3[3 * i + k];
  }
  if (a.onehots != nullptr) {
    float* oh = a.onehots + (long long)a.r.n_classes * o;
    for (int k = 0; k < a.r.n_classes; k++) oh[k] = k == ci ? 1.0f : 0.0f;
  }
  if (a.batch != nullptr || a.group != nullptr) {
    const size_t w = (size_t)model * a.n_words + (b >> 5);
    const uint32_t bit = 1u << (b & 31), below = bit - 1u, p = a.presence[w];
    if (a.batch != nullptr) a.batch[o] = (int32_t)(a.rank_b[w] + (uint32_t)__popc(p & below));
    if (a.group != nullptr) {
      const uint32_t h = a.has[b >> 5];
      a.group[o] = (h & bit) ? (int32_t)(a.rank_g[w] + (uint32_t)__popc(p & h & below)) : -1;
    }
  }
}

// grid (K, 3), one wave per (instance rank, model): the model's instances with a code, ascending, and their codes
struct SplitCodesArgs {
  const uint32_t *presence, *has, *rank_g;
  int n_words;
  const int16_t* instances;
  long long K;
  const float* lut;
  int n_lut, z_dim;
  long long g_base[MS_MODELS], n_groups;
  int16_t* group_instances;
  float* codes;
};
__global__ __launch_bounds__(64) void k_split_codes(const SplitCodesArgs a) {
  const long long rk = blockIdx.x;
  const int m = blockIdx.y;
  const size_t w = (size_t)m * a.n_words + (size_t)(rk >> 5);
  const uint32_t bit = 1u << (rk & 31), sel = a.presence[w] & a.has[rk >> 5];
  if (rk >= a.K || !(sel & bit)) return;
  const long long gm = a.rank_g[w] + (uint32_t)__popc(sel & (bit - 1u));
  const long long g = (m == 0 ? a.g_base[0] : (m == 1 ? a.g_base[1] : a.g_base[2])) + gm;
  const int id = a.instances[rk];
  if (g >= a.n_groups || id < 0 || id >= a.n_lut) return;  // a stale workspace or count stays in bounds
  if (a.group_instances != nullptr && threadIdx.x == 0) a.group_instances[g] = (int16_t)id;
  if (a.codes != nullptr)
    for (int j = threadIdx.x; j < a.z_dim; j += 64) a.codes[g * a.z_dim + j] = a.lut[(long long)id * a.z_dim + j];
}

// ---- K18 ----
struct Points14Args {
  const float *xyz, *scales;
  long long xyz_stride, scales_stride, n;
  gcv_gaussian_attrs at;  // segments without rows have n = 0
  float* out;
};
__global__ __launch_bounds__(256) void k_points14(const Points14Args a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  long long j = i;
  const float *rgb = a.at.seg[0].rgb, *dxyz = a.at.seg[0].dxyz, *scale = a.at.seg[0].scale, *opacity = a.at.seg[0].opacity;
  if (j >= a.at.seg[0].n) {
    j -= a.at.seg[0].n;
    rgb = a.at.seg[1].rgb; dxyz = a.at.seg[1].dxyz; scale = a.at.seg[1].scale; opacity = a.at.seg[1].opacity;
    if (j >= a.at.seg[1].n) {
      j -= a.at.seg[1].n;
      rgb = a.at.seg[2].rgb; dxyz = a.at.seg[2].dxyz; scale = a.at.seg[2].scale; opacity = a.at.seg[2].opacity;
    }
  }
  const float* p = a.xyz + a.xyz_stride * i;
  const float* s = a.scales + a.scales_stride * i;
  float x = p[0], y = p[1], z = p[2], sx = s[0], sy = s[1], sz = s[2];
  if (dxyz != nullptr) { x += dxyz[3 * j]; y += dxyz[3 * j + 1]; z += dxyz[3 * j + 2]; }
  if (scale != nullptr) { sx *= scale[3 * j]; sy *= scale[3 * j + 1]; sz *= scale[3 * j + 2]; }
  const float op = opacity != nullptr ? opacity[j] : 1.0f;
  float2* o = reinterpret_cast<float2*>(a.out + 14 * i);  // 56-byte rows: 8-byte aligned
  o[0] = make_float2(x, y);
  o[1] = make_float2(z, op);
  o[2] = make_float2(sx, sy);
  o[3] = make_float2(sz, 1.0f);
  o[4] = make_float2(0.0f, 0.0f);
  o[5] = make_float2(0.0f, rgb[3 * j]);
  o[6] = make_float2(rgb[3 * j + 1], rgb[3 * j + 2]);
}

// the argument checks gcv_model_split_count and gcv_model_split_emit share; nothing is queued before they pass
int split_check(const float* classes, const int32_t* batch_index, int64_t M, const int16_t* instances, int64_t K,
                const uint8_t* lut_has, int32_t n_lut, const gcv_model_rule* rule, const void* workspace,
                size_t workspace_bytes, SplitRule* out) {
  if (M < 0 || K < 0 || n_lut < 0)
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: n_visible, n_instances and n_lut must not be negative");
  if (M >= 2147483648ll || K > MS_MAX_INSTANCES)
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: n_visible must be below 2^31 and n_instances at most 65536");
  if (!workspace || !rule || (M > 0 && (!classes || !batch_index)) || (K > 0 && !instances) || (n_lut > 0 && !lut_has))
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: null classes / batch_index / instances / lut_has / rule / workspace");
  if (misaligned(classes, 4) || misaligned(batch_index, 4) || misaligned(instances, 2) || misaligned(workspace, 16))
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: misaligned classes / batch_index / instances / workspace (16 bytes)");
  if (rule->n_classes < 1 || rule->n_classes > 32)
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: n_classes must be in [1, 32]");
  if (!(rule->proj_size == rule->proj_size) || rule->proj_size == 0.0f)
    return fail(GCV_ERR_INVALID_ARGUMENT, "model split: proj_size must be a non-zero number");
  out->n_classes = rule->n_classes;
  out->model_bits = 0ull;
  for (int c = 0; c < rule->n_classes; c++) {
    const int m = rule->model_of_class[c];
    if (m < -1 || m >= MS_MODELS) return fail(GCV_ERR_INVALID_ARGUMENT, "model split: model_of_class must be -1, 0, 1 or 2");
    out->model_bits |= (unsigned long long)(m < 0 ? 3 : m) << (2 * c);
  }
  out->tlp_x = rule->proj_tlp[0];
  out->tlp_y = rule->proj_tlp[1];
  out->size = rule->proj_size;
  if (workspace_bytes < split_layout(M, K).total) return fail(GCV_ERR_BUFFER_TOO_SMALL, "model split workspace too small");
  return 0;
}

}  // namespace

extern "C" {

int gcv_model_split_models(void) { return MS_MODELS; }

size_t gcv_model_split_workspace_bytes(int64_t n_visible, int64_t n_instances) {
  if (n_visible < 0 || n_instances < 0 || n_visible >= 2147483648ll || n_instances > MS_MAX_INSTANCES) {
    fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_workspace_bytes: n_visible must be in [0, 2^31), n_instances in [0, 65536]");
    return 0;
  }
  return split_layout(n_visible, n_instances).total;
}

int gcv_model_split_count(const float* classes, const int32_t* batch_index, int64_t M, const int16_t* instances, int64_t K,
                          const uint8_t* lut_has, int32_t n_lut, const gcv_model_rule* rule, void* workspace,
                          size_t workspace_bytes, int64_t counts_host[9], void* hip_stream) {
  SplitRule r;
  if (int rc = split_check(classes, batch_index, M, instances, K, lut_has, n_lut, rule, workspace, workspace_bytes, &r)) return rc;
  if (!counts_host) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_count: null counts_host");
  hipStream_t s = (hipStream_t)hip_stream;
  const SplitLayout l = split_layout(M, K);
  char* ws = (char*)workspace;
  uint32_t* head = (uint32_t*)ws;
  uint32_t *presence = (uint32_t*)(ws + l.presence), *sums = (uint32_t*)(ws + l.sums);
  HIP_TRY(hipMemsetAsync(ws, 0, l.has, s), "model split workspace clear");  // head and presence tables
  if (l.n_blocks > 0)
    k_split_count<<<(unsigned)l.n_blocks, MS_BLOCK, 0, s>>>(classes, batch_index, (long long)M, (long long)K, r, presence,
                                                            l.n_words, sums, head);
  k_split_scan<<<1, 1024, 0, s>>>(sums, l.n_blocks, presence, l.n_words, instances, (long long)K, lut_has, n_lut,
                                  (uint32_t*)(ws + l.has), (uint32_t*)(ws + l.rank_b), (uint32_t*)(ws + l.rank_g), head);
  HIP_TRY(hipGetLastError(), "model split count launch");
  uint32_t h[MS_HEAD_WORDS];
  HIP_TRY(hipMemcpyAsync(h, head, sizeof(h), hipMemcpyDeviceToHost, s), "model split count read-back");
  HIP_TRY(hipStreamSynchronize(s), "model split count sync");
  if (h[MS_HEAD_BAD] != 0u) {
    char msg[200];
    snprintf(msg, sizeof(msg), "model split: %u row(s) whose class is not an integer in [0, %d) or whose batch_index is outside [0, %lld)",
             h[MS_HEAD_BAD], (int)rule->n_classes, (long long)K);
    return fail(GCV_ERR_INVALID_ARGUMENT, msg);
  }
  for (int k = 0; k < 9; k++) counts_host[k] = (int64_t)h[k];
  return 0;
}

int gcv_model_split_emit(const float* classes, const int32_t* batch_index, const float* points8, const float* scales3,
                         int64_t M, const int16_t* instances, int64_t K, const uint8_t* lut_has, const float* lut,
                         int32_t n_lut, int32_t z_dim, const gcv_model_rule* rule, const void* workspace,
                         size_t workspace_bytes, const int64_t counts_host[9], int64_t* index_out, float* points8_out,
                         int32_t* batch_out, float* classes_out, float* scales3_out, float* onehots_out, float* proj_uv_out,
                         int32_t* group_out, int16_t* group_instances_out, float* codes_out, void* hip_stream) {
  SplitRule r;
  if (int rc = split_check(classes, batch_index, M, instances, K, lut_has, n_lut, rule, workspace, workspace_bytes, &r)) return rc;
  if (!counts_host) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: null counts_host");
  long long N = 0, G = 0;
  for (int m = 0; m < MS_MODELS; m++) {
    const int64_t n = counts_host[m], b = counts_host[3 + m], g = counts_host[6 + m];
    if (n < 0 || b < 0 || g < 0 || n > M || g > b || b > K || b > n)
      return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: counts need 0 <= G_m <= B_m <= min(n_m, n_instances), n_m <= n_visible");
    N += n;
    G += g;
  }
  if (N > M) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: n_0 + n_1 + n_2 exceeds n_visible");
  if (z_dim < 0) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: negative z_dim");
  if (N == 0) return 0;
  if ((points8_out || proj_uv_out) && !points8) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: null points8");
  if (scales3_out && !scales3) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: null scales3");
  if (codes_out && G > 0 && z_dim > 0 && !lut) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: null lut");
  if (misaligned(points8, 16) || misaligned(scales3, 4) || misaligned(lut, 4) || misaligned(index_out, 8) ||
      misaligned(points8_out, 16) || misaligned(batch_out, 4) || misaligned(classes_out, 4) || misaligned(scales3_out, 4) ||
      misaligned(onehots_out, 4) || misaligned(proj_uv_out, 4) || misaligned(group_out, 4) || misaligned(group_instances_out, 2) ||
      misaligned(codes_out, 4))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_model_split_emit: misaligned input or output (points8 needs 16 bytes)");
  hipStream_t s = (hipStream_t)hip_stream;
  const SplitLayout l = split_layout(M, K);
  const char* ws = (const char*)workspace;
  SplitEmitArgs a;
  a.classes = classes; a.points8 = points8; a.scales3 = scales3; a.batch_index = batch_index;
  a.M = M; a.K = K; a.N = N; a.r = r;
  a.presence = (const uint32_t*)(ws + l.presence); a.has = (const uint32_t*)(ws + l.has);
  a.rank_b = (const uint32_t*)(ws + l.rank_b); a.rank_g = (const uint32_t*)(ws + l.rank_g);
  a.sums = (const uint32_t*)(ws + l.sums); a.n_words = l.n_words;
  a.index = (long long*)index_out; a.points8_out = points8_out; a.classes_out = classes_out; a.scales3_out = scales3_out;
  a.onehots = onehots_out; a.proj_uv = proj_uv_out; a.batch = batch_out; a.group = group_out;
  k_split_emit<<<(unsigned)l.n_blocks, MS_BLOCK, 0, s>>>(a);
  if (G > 0 && K > 0 && (group_instances_out || codes_out)) {
    SplitCodesArgs c;
    c.presence = a.presence; c.has = a.has; c.rank_g = a.rank_g; c.n_words = l.n_words;
    c.instances = instances; c.K = K; c.lut = lut; c.n_lut = n_lut; c.z_dim = z_dim;
    c.g_base[0] = 0; c.g_base[1] = counts_host[6]; c.g_base[2] = counts_host[6] + counts_host[7];
    c.n_groups = G; c.group_instances = group_instances_out; c.codes = codes_out;
    k_split_codes<<<dim3((unsigned)K, MS_MODELS), 64, 0, s>>>(c);
  }
  HIP_TRY(hipGetLastError(), "model split emit launch");
  return 0;
}

int gcv_gaussian_points(const float* xyz, int64_t xyz_stride, const float* scales, int64_t scales_stride, int64_t n,
                 gcv_gaussian_attrs attrs, float* out, void* hip_stream) {
  if (n < 0 || n >= 2147483648ll) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: n must be in [0, 2^31)");
  if (attrs.n_segments < 1 || attrs.n_segments > 3) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: 1 to 3 segments");
  if (xyz_stride < 3 || scales_stride < 3) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: row strides must be at least 3");
  Points14Args a;
  long long total = 0;
  int with_rows = 0, has_dxyz = 0, has_scale = 0, has_opacity = 0;
  for (int k = 0; k < 3; k++) {
    gcv_gaussian_segment& g = a.at.seg[k];
    g = attrs.seg[k];
    if (k >= attrs.n_segments || g.n == 0) {
      g.n = 0;
      g.rgb = g.dxyz = g.scale = g.opacity = nullptr;
      continue;
    }
    if (g.n < 0) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: negative segment size");
    if (!g.rgb) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: null rgb");
    if (misaligned(g.rgb, 4) || misaligned(g.dxyz, 4) || misaligned(g.scale, 4) || misaligned(g.opacity, 4))
      return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: misaligned attribute pointer");
    total += g.n;
    with_rows++;
    has_dxyz += g.dxyz != nullptr;
    has_scale += g.scale != nullptr;
    has_opacity += g.opacity != nullptr;
  }
  a.at.n_segments = attrs.n_segments;
  if (total != n) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: the segments' rows do not add up to n");
  if ((has_dxyz && has_dxyz != with_rows) || (has_scale && has_scale != with_rows) || (has_opacity && has_opacity != with_rows))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: a key must be present in every segment or in none");
  if (n == 0) return 0;
  if (!xyz || !scales || !out) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: null xyz / scales / out");
  if (misaligned(xyz, 4) || misaligned(scales, 4) || misaligned(out, 8))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gaussian_points: misaligned xyz / scales / out (8 bytes)");
  a.xyz = xyz; a.scales = scales; a.xyz_stride = xyz_stride; a.scales_stride = scales_stride; a.n = n; a.out = out;
  k_points14<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)hip_stream>>>(a);
  HIP_TRY(hipGetLastError(), "points14 launch");
  return 0;
}

}  // extern "C"
