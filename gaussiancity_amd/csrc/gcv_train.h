// gcv_train.h -- K23 (distinct instances of a training crop) and K24 (the generator's inputs of a training step in one
// launch) of libgcv_hip.so; included by gcv_points.hip, whose helpers (fail, HIP_TRY, misaligned, vs_block_excl_scan) it
// uses.  Reference behaviour: core/train.py:207-224 with utils/datasets.py:265-282 / :333-352 (instances_to_classes),
// utils/helpers.py:197-223 (get_point_scales), :127-133 (get_one_hot), :183-194 (get_projection_uv), :136-155 (get_z).
//
// K16 / K17's shape once more -- prefix counts over a presence table, here one bit per instance id in [0, 32768):
//   mark   one thread per row: the row's instance id from column 4; an atomic OR of its bit (a lane whose left neighbour
//          holds the same id leaves the bit to it); the rows whose id is no integer in [0, 32768) are counted;
//   scan   one 1024-thread block, one presence word per thread: the rank of each word's first instance -> the word
//          prefix, and I;
//   emit   one thread per row: the row is read once and every output written from it.  With groups the table and its
//          word prefix (8 KB) are staged in LDS: a row's group = prefix[word] + the bits below its own.  Block 0 also
//          writes the I ids.  The last block to finish (a ticket) stores the number of flagged rows as the flag word and
//          leaves the ticket and the counter zero again, so an emit needs no clear in front of it.
// Integer work except scale * scale_factor (one fp32 multiply) and proj_uv (three fp32 operations in upstream's order,
// IEEE division, no contraction).  No float atomics; the order-free operations are the bit ORs and the counters.
#pragma once

namespace {

constexpr int TI_BLOCK = 256;
constexpr int TI_MAX_INSTANCE = 32768;            // dataset_generator.py:1315 asserts below it; get_z casts to int16
constexpr int TI_WORDS = TI_MAX_INSTANCE / 32;    // 1024 presence words, 4 KB
constexpr int TI_MAX_CLASSES = 32;
// head words (uint32); the flag word's place is part of the ABI (include/gcv.h: GCV_TRAIN_INPUTS_FLAG_OFFSET)
enum { TI_HEAD_I = 0, TI_HEAD_BAD = 1, TI_HEAD_FLAG = 2, TI_HEAD_EMIT_BAD = 3, TI_HEAD_TICKET = 4, TI_HEAD_WORDS = 64 };
static_assert(TI_HEAD_FLAG * sizeof(uint32_t) == GCV_TRAIN_INPUTS_FLAG_OFFSET, "the flag word's documented offset");
static_assert(TI_WORDS == 4 * TI_BLOCK, "the emit stages four words per thread; the scan has one word per thread of 1024");

// workspace: [head u32 x 64][presence u32 x 1024] -- cleared by every count -- then [word prefix u32 x 1024]
constexpr size_t TI_OFF_PRESENCE = sizeof(uint32_t) * TI_HEAD_WORDS;
constexpr size_t TI_OFF_PREFIX = TI_OFF_PRESENCE + sizeof(uint32_t) * TI_WORDS;
constexpr size_t TI_WORKSPACE = TI_OFF_PREFIX + sizeof(uint32_t) * TI_WORDS;

// the instance id of a row, -1 when it is no integer in [0, 32768) (a NaN fails the comparisons)
__device__ __forceinline__ int ti_instance(float f) {
  if (!(f >= 0.0f && f < (float)TI_MAX_INSTANCE)) return -1;
  const int i = (int)f;
  return (float)i == f ? i : -1;
}

__global__ __launch_bounds__(TI_BLOCK) void k_train_mark(const float* __restrict__ pts, long long stride, long long n,
                                                         uint32_t* __restrict__ presence, uint32_t* __restrict__ head) {
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * TI_BLOCK + tid;
  int id = -2;  // -2: no row, -1: a flagged row
  if (i < n) id = ti_instance(pts[i * stride + 4]);
  const int left = __shfl_up(id, 1, 64);
  if (id >= 0 && ((tid & 63) == 0 || left != id)) atomicOr(&presence[id >> 5], 1u << (id & 31));
  const unsigned long long bad = __ballot(id == -1);
  if ((tid & 63) == 0 && bad != 0ull) atomicAdd(&head[TI_HEAD_BAD], (uint32_t)__popcll(bad));
}

__global__ __launch_bounds__(1024) void k_train_scan(const uint32_t* __restrict__ presence, uint32_t* __restrict__ prefix,
                                                     uint32_t* __restrict__ head) {
  __shared__ uint32_t lds16[16];
  const int tid = threadIdx.x;
  uint32_t total;
  const uint32_t r = vs_block_excl_scan<16>((uint32_t)__popc(presence[tid]), lds16, &total);
  prefix[tid] = r;
  if (tid == 0) head[TI_HEAD_I] = total;
}

struct TrainRule {
  float bldg_min, bldg_max, car_min, car_max;  // the bounds as the float a comparison with a float tensor sees
  float facade, roof, car;
  int n_classes;
  uint32_t special;
  float scale_factor, proj_size;
};

struct TrainEmitArgs {
  const float* pts;
  long long stride, n, rows_per_batch, n_instances;
  TrainRule r;
  const float* tlp;
  uint32_t* head;
  const uint32_t *presence, *prefix;
  int with_groups, onehot_vec4;
  float *classes, *scales3, *onehots, *proj_uv;
  long long* batch;
  int32_t* group;
  int16_t* group_instances;
};

// instances_to_classes on the float id: facade, roof and car masks from the id itself, assigned in that order
// (torch's % on floats is the floored remainder)
__device__ __forceinline__ float ti_class(const TrainRule& r, float f) {
  float c = f;
  if (f >= r.bldg_min && f < r.bldg_max) {
    float m = fmodf(f, 2.0f);
    if (m < 0.0f) m += 2.0f;
    if (m == 0.0f) c = r.facade;
    if (m == 1.0f) c = r.roof;
  }
  if (f >= r.car_min && f < r.car_max) c = r.car;
  return c;
}

__global__ __launch_bounds__(TI_BLOCK) void k_train_emit(const TrainEmitArgs a) {
  __shared__ __align__(16) uint32_t s_presence[TI_WORDS], s_prefix[TI_WORDS];
  __shared__ uint32_t s_bad[TI_BLOCK / 64];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * TI_BLOCK + tid;
  if (a.with_groups) {
    *reinterpret_cast<uint4*>(&s_presence[4 * tid]) = *reinterpret_cast<const uint4*>(a.presence + 4 * tid);
    *reinterpret_cast<uint4*>(&s_prefix[4 * tid]) = *reinterpret_cast<const uint4*>(a.prefix + 4 * tid);
    __syncthreads();
    if (blockIdx.x == 0 && a.group_instances != nullptr) {  // the I ids, ascending
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int w = 4 * tid + j;
        uint32_t p = s_presence[w];
        long long g = s_prefix[w];
        while (p) {
          const int bit = __ffs((int)p) - 1;
          p &= p - 1;
          if (g < a.n_instances) a.group_instances[g] = (int16_t)(32 * w + bit);  // a stale count stays in bounds
          g++;
        }
      }
    }
  }
  bool flagged = false;
  if (i < a.n) {
    const float* row = a.pts + i * a.stride;
    const float f = row[4];
    const int id = ti_instance(f);
    const float c = ti_class(a.r, f);
    int ci = -1;  // the class as an index, -1: no integer in [0, n_classes)
    if (c >= 0.0f && c < (float)a.r.n_classes) {
      ci = (int)c;
      if ((float)ci != c) ci = -1;
    }
    flagged = id < 0 || ci < 0;
    if (a.classes != nullptr) a.classes[i] = c;
    if (a.scales3 != nullptr) {  // get_point_scales: ones * scales, then z = 1 where the class is special
      const float s = row[3] * a.r.scale_factor;
      bool special = false;
      if (c >= 0.0f && c < (float)TI_MAX_CLASSES) {
        const int k = (int)c;
        special = (float)k == c && ((a.r.special >> k) & 1u) != 0u;
      }
      a.scales3[3 * i] = s;
      a.scales3[3 * i + 1] = s;
      a.scales3[3 * i + 2] = special ? 1.0f : s;
    }
    if (a.onehots != nullptr) {
      const int hot = flagged ? -1 : ci;
      float* oh = a.onehots + (long long)a.r.n_classes * i;
      if (a.onehot_vec4) {
        for (int k = 0; k < a.r.n_classes; k += 4)
          *reinterpret_cast<float4*>(oh + k) = make_float4(k == hot ? 1.0f : 0.0f, k + 1 == hot ? 1.0f : 0.0f,
                                                           k + 2 == hot ? 1.0f : 0.0f, k + 3 == hot ? 1.0f : 0.0f);
      } else {
        for (int k = 0; k < a.r.n_classes; k++) oh[k] = k == hot ? 1.0f : 0.0f;
      }
    }
    if (a.proj_uv != nullptr) {  // utils/helpers.py:188-194: subtract, divide, times 2, minus 1
      float tx = 0.0f, ty = 0.0f;
      if (a.tlp != nullptr) {
        const long long b = i / a.rows_per_batch;
        tx = a.tlp[2 * b];
        ty = a.tlp[2 * b + 1];
      }
      a.proj_uv[2 * i] = ((row[0] - tx) / a.r.proj_size) * 2.0f - 1.0f;
      a.proj_uv[2 * i + 1] = ((row[1] - ty) / a.r.proj_size) * 2.0f - 1.0f;
    }
    if (a.batch != nullptr) a.batch[i] = (long long)row[8];
    if (a.with_groups && a.group != nullptr) {
      int g = -1;
      if (!flagged) {
        const int w = id >> 5;
        g = (int)(s_prefix[w] + (uint32_t)__popc(s_presence[w] & ((1u << (id & 31)) - 1u)));
      }
      a.group[i] = g;
    }
  }
  // the flag word: the block's flagged rows into the counter, then the ticket; the last block stores the total
  const unsigned long long bad = __ballot(flagged);
  if ((tid & 63) == 0) s_bad[tid >> 6] = (uint32_t)__popcll(bad);
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < TI_BLOCK / 64; w++) s += s_bad[w];
    if (s) atomicAdd(&a.head[TI_HEAD_EMIT_BAD], s);
    __threadfence();
    const uint32_t t = atomicAdd(&a.head[TI_HEAD_TICKET], 1u);
    if (t == gridDim.x - 1) {
      __threadfence();
      a.head[TI_HEAD_FLAG] = atomicExch(&a.head[TI_HEAD_EMIT_BAD], 0u);
      atomicExch(&a.head[TI_HEAD_TICKET], 0u);
    }
  }
}

// the argument checks gcv_train_inputs_count and gcv_train_inputs_emit share; nothing is queued before they pass
int train_check(const char* who, const float* pts, int64_t row_stride, int64_t n_rows, const void* workspace,
                size_t workspace_bytes) {
  char msg[160];
  const char* what = nullptr;
  if (n_rows < 0 || n_rows >= 2147483648ll) what = "n_rows must be in [0, 2^31)";
  else if (row_stride < 9) what = "row_stride must be at least 9 elements";
  else if (!workspace || (n_rows > 0 && !pts)) what = "null pts / workspace";
  else if (misaligned(pts, 4) || misaligned(workspace, 16)) what = "misaligned pts / workspace (16 bytes)";
  else if (workspace_bytes < TI_WORKSPACE) what = "workspace too small";
  if (!what) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return fail(GCV_ERR_INVALID_ARGUMENT, msg);
}

}  // namespace

extern "C" {

int gcv_train_inputs_max_classes(void) { return TI_MAX_CLASSES; }

size_t gcv_train_inputs_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows >= 2147483648ll) {
    fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_workspace_bytes: n_rows must be in [0, 2^31)");
    return 0;
  }
  return TI_WORKSPACE;
}

int gcv_train_inputs_count(const float* pts, int64_t row_stride, int64_t n_rows, void* workspace, size_t workspace_bytes,
                           int64_t counts_host[2], void* hip_stream) {
  if (int rc = train_check("gcv_train_inputs_count", pts, row_stride, n_rows, workspace, workspace_bytes)) return rc;
  if (!counts_host) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_count: null counts_host");
  hipStream_t s = (hipStream_t)hip_stream;
  char* ws = (char*)workspace;
  uint32_t *head = (uint32_t*)ws, *presence = (uint32_t*)(ws + TI_OFF_PRESENCE);
  HIP_TRY(hipMemsetAsync(ws, 0, TI_OFF_PREFIX, s), "train inputs workspace clear");  // head and presence table
  const long long n_blocks = (n_rows + TI_BLOCK - 1) / TI_BLOCK;
  if (n_blocks > 0) k_train_mark<<<(unsigned)n_blocks, TI_BLOCK, 0, s>>>(pts, (long long)row_stride, (long long)n_rows, presence, head);
  k_train_scan<<<1, 1024, 0, s>>>(presence, (uint32_t*)(ws + TI_OFF_PREFIX), head);
  HIP_TRY(hipGetLastError(), "train inputs count launch");
  uint32_t h[2];
  HIP_TRY(hipMemcpyAsync(h, head, sizeof(h), hipMemcpyDeviceToHost, s), "train inputs count read-back");
  HIP_TRY(hipStreamSynchronize(s), "train inputs count sync");
  counts_host[0] = (int64_t)h[TI_HEAD_I];
  counts_host[1] = (int64_t)h[TI_HEAD_BAD];
  return 0;
}

int gcv_train_inputs_emit(const float* pts, int64_t row_stride, int64_t n_rows, int64_t rows_per_batch,
                          const gcv_train_rule* rule, const float* proj_tlp, void* workspace, size_t workspace_bytes,
                          int32_t with_groups, int64_t n_instances, float* classes, float* scales3, float* onehots,
                          float* proj_uv, int64_t* batch, int32_t* group, int16_t* group_instances, void* hip_stream) {
  const char* who = "gcv_train_inputs_emit";
  if (int rc = train_check(who, pts, row_stride, n_rows, workspace, workspace_bytes)) return rc;
  if (!rule) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: null rule_host");
  if (rule->n_classes < 1 || rule->n_classes > TI_MAX_CLASSES)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: n_classes must be in [1, 32]");
  if (!(rule->proj_size == rule->proj_size) || rule->proj_size == 0.0f)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: proj_size must be a non-zero number");
  if (rows_per_batch < 0 || (n_rows > 0 && (rows_per_batch < 1 || n_rows % rows_per_batch != 0)))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: rows_per_batch must divide n_rows");
  if (with_groups && (n_instances < 0 || n_instances > TI_MAX_INSTANCE || n_instances > n_rows))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: n_instances must be in [0, min(n_rows, 32768)]");
  if (with_groups && n_instances > 0 && !group_instances)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: null group_instances");
  if (misaligned(proj_tlp, 4) || misaligned(classes, 4) || misaligned(scales3, 4) || misaligned(onehots, 4) ||
      misaligned(proj_uv, 4) || misaligned(batch, 8) || misaligned(group, 4) || misaligned(group_instances, 2))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_train_inputs_emit: misaligned proj_tlp or output");
  if (n_rows == 0) return 0;
  char* ws = (char*)workspace;
  TrainEmitArgs a;
  a.pts = pts; a.stride = row_stride; a.n = n_rows; a.rows_per_batch = rows_per_batch; a.n_instances = n_instances;
  a.r.bldg_min = (float)rule->bldg_ins_min; a.r.bldg_max = (float)rule->bldg_ins_max;
  a.r.car_min = (float)rule->car_ins_min; a.r.car_max = (float)rule->car_ins_max;
  a.r.facade = (float)rule->facade_class; a.r.roof = (float)rule->roof_class; a.r.car = (float)rule->car_class;
  a.r.n_classes = rule->n_classes; a.r.special = rule->special_z_classes;
  a.r.scale_factor = rule->scale_factor; a.r.proj_size = rule->proj_size;
  a.tlp = proj_tlp; a.head = (uint32_t*)ws;
  a.presence = (const uint32_t*)(ws + TI_OFF_PRESENCE); a.prefix = (const uint32_t*)(ws + TI_OFF_PREFIX);
  a.with_groups = with_groups != 0; a.onehot_vec4 = rule->n_classes % 4 == 0 && !misaligned(onehots, 16);
  a.classes = classes; a.scales3 = scales3; a.onehots = onehots; a.proj_uv = proj_uv; a.batch = (long long*)batch;
  a.group = group; a.group_instances = group_instances;
  k_train_emit<<<(unsigned)((n_rows + TI_BLOCK - 1) / TI_BLOCK), TI_BLOCK, 0, (hipStream_t)hip_stream>>>(a);
  HIP_TRY(hipGetLastError(), "train inputs emit launch");
  return 0;
}

}  // extern "C"
