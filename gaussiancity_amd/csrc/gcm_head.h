// gcm_head.h -- the attribute head's output layers in a training step (gcm_head_train_*): for up to
// four keys the last Linear (C = 1 or 3 outputs), the output transform, the rows without a group and, on request, the
// rasterizer's [N][14] record in ONE launch, and a backward of two launches without float atomics.  Included by
// gcm_modlinear.hip after gcm_tile.h; kernels and the plan only, the C ABI functions are at the end of that file.
//
// Forward (k_head_train_fwd): k_head_out's row sum -- 16 lanes per row, lane q chains the elements 4 q + 64 k .. + 3 with k
// ascending, then the fixed exchange tree (8, 4, 2, 1 lanes apart) -- written out again here operation for operation, so a
// value has gcm_head_out's bits.  After the tree all 16 lanes hold the sum; lane c < C adds the bias, stores `pre` and
// applies the transform in double, so the exps of a row spread over up to 10 lanes; the [N][14] record is put together
// from a row's values in LDS by the lanes 0 .. 13, one column each.
//
// Backward, row side (k_head_train_rows, grid = (row blocks, keys)): per tile of 64 rows the workgroup stages
// dv = dout o T'(pre) and the row's "has a group" in LDS (T' in double from the stored pre), then the threads walk the rows
// in ascending order: a thread owns 4 columns of I (at most 128 threads per row: I <= 512) and half of the tile's rows, holds
// its W columns in registers, loads h 8 rows at a time, stores dh = sum_c dv_c W_c and chains dW += dv_c h.  The two halves
// are added (rows 0..31, then 32..63) and the block's tiles follow one another in the same registers, so the block leaves ONE
// record [C][I] + [C] (dW, db) however many tiles it walked.
// Backward, fold (k_head_train_fold, grid = (element blocks, keys)): an element's records are cut into kHeadFoldGroups
// contiguous groups; 16 lanes chain one group each in ascending record order, then one lane adds the groups in ascending
// order, both in double with one rounding at the end (the records are float32; db's chain inside a block is double too).  Records, groups and tiles per block depend on N alone (head_train_plan): the bits do not depend on the device's
// occupancy, the stream or what the workspace held.
#pragma once

namespace {

constexpr int kHeadTrainMaxIn = 512;      // 128 threads x 4 columns own a row
constexpr int kHeadPreFloats = 10;        // a row of pre: xyz 0..2, rgb 3..5, scale 6..8, opacity 9
constexpr int kHeadMaxRecords = 1024;     // row blocks of the backward: beyond 65 536 rows a block walks several tiles
constexpr int kHeadFoldGroups = 16;       // first level of the fold

struct HeadKeys {
  gcm_head_key k[4];
  int n;
};

__host__ __device__ __forceinline__ int head_channels(int kind) { return kind == GCM_OPACITY ? 1 : 3; }
__host__ __device__ __forceinline__ int head_pre_at(int kind) { return kind * 3; }  // opacity is kind 3: column 9
// a key's columns of the rasterizer's record: xyz 0..2, opacity 3, scale 4..6, (rotation 7..10), rgb 11..13
__host__ __device__ __forceinline__ int head_p14_at(int kind) {
  return kind == GCM_XYZ ? 0 : kind == GCM_OPACITY ? 3 : kind == GCM_SCALE ? 4 : 11;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_train_fwd(const HeadKeys keys, const int32_t* __restrict__ group, int64_t N, int I,
                                                        float* __restrict__ pre, const float* __restrict__ xyz, int64_t xs,
                                                        const float* __restrict__ scales, int64_t ss, float* __restrict__ p14) {
  __shared__ float attr[16][12];  // a row's transformed values at head_pre_at(kind) + c, for the [N][14] record
  const int q = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int64_t row = (int64_t)blockIdx.x * 16 + rl;
  const bool live = row < N;
  const int gr = !live ? -1 : (group ? (group[row] >= 0 ? 0 : -1) : 0);
  int has = 0;  // bit per kind
  for (int kk = 0; kk < keys.n; kk++) {
    const gcm_head_key& key = keys.k[kk];
    const int kind = key.kind, nc = head_channels(kind);
    const float* __restrict__ f = key.h;
    const float* __restrict__ w = key.w;
    has |= 1 << kind;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (gr >= 0) {
      for (int i = 4 * q; i < I; i += 64) {
        const f4 v = ld4(f + row * key.h_stride + i);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          if (c < nc) {
            const f4 wv = ld4(w + (int64_t)c * I + i);
#pragma unroll
            for (int k = 0; k < 4; k++) acc[c] += v[k] * wv[k];
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int m = 8; m >= 1; m >>= 1) acc[c] += __shfl_xor(acc[c], m, 64);
    if (live && q < nc) {
      const float a = q == 0 ? acc[0] : (q == 1 ? acc[1] : acc[2]);
      float res = 0.0f, v = 0.0f;
      if (gr >= 0) {
        v = key.b ? a + key.b[q] : a;
        const double sg = 1.0 / (1.0 + exp(-(double)v));
        double d;
        if (kind == GCM_SCALE) d = 1.0 + (double)fminf(fmaxf(v, -1.0f), 1.0f) * (double)key.factor;
        else if (kind == GCM_OPACITY) d = sg * (double)key.factor + (1.0 - (double)key.factor);
        else d = (sg - 0.5) * (double)key.factor;
        res = (float)d;
      }
      if (pre) pre[row * kHeadPreFloats + head_pre_at(kind) + q] = v;
      if (p14) attr[rl][head_pre_at(kind) + q] = res;
      else key.out[row * key.out_stride + q] = res;
    }
  }
  if (!p14) return;
  __syncthreads();
  if (!live || q >= 14) return;
  float v;
  if (q < 3) {
    v = xyz[row * xs + q];
    if ((has >> GCM_XYZ & 1)) v = v + attr[rl][head_pre_at(GCM_XYZ) + q];
  } else if (q == 3) {
    v = (has >> GCM_OPACITY & 1) ? attr[rl][head_pre_at(GCM_OPACITY)] : 1.0f;
  } else if (q < 7) {
    v = scales[row * ss + (q - 4)];
    if ((has >> GCM_SCALE & 1)) v = v * attr[rl][head_pre_at(GCM_SCALE) + (q - 4)];
  } else if (q < 11) {
    v = q == 7 ? 1.0f : 0.0f;
  } else {
    v = attr[rl][head_pre_at(GCM_RGB) + (q - 11)];
  }
  p14[row * 14 + q] = v;
}

// ---- backward, row side -----------------------------------------------------------------------------------------------
// record of a (key, block): dW [C][I], then db [C]; records are `rec_floats` apart, a key's block of records `key_floats`.
__global__ __launch_bounds__(256) void k_head_train_rows(const HeadKeys keys, const int32_t* __restrict__ group, int64_t N, int I,
                                                         const float* __restrict__ pre, const float* __restrict__ scales,
                                                         int64_t ss, const float* __restrict__ dp, int64_t dps, int64_t tiles,
                                                         int tpb, int64_t rec_floats, int64_t key_floats,
                                                         float* __restrict__ records) {
  __shared__ f4 dvs[64];        // dv of the tile's rows; .w: 1 for a row that has a group, 0 otherwise
  __shared__ f4 half1[3][128];  // the upper half's dW, to be added to the lower half's
  const gcm_head_key& key = keys.k[blockIdx.y];
  const int kind = key.kind, nc = head_channels(kind);
  float* __restrict__ dh = key.dh;
  const bool want_w = key.dw != nullptr, want_b = key.db != nullptr;
  if (!dh && !want_w && !want_b) return;
  const float* __restrict__ h = key.h;
  const int tid = threadIdx.x, ct = tid & 127, rh = tid >> 7, i0 = 4 * ct;
  const bool cols = i0 < I;
  f4 w[3] = {zero4(), zero4(), zero4()}, aw[3] = {zero4(), zero4(), zero4()};
  if (cols && dh)
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (c < nc) w[c] = ld4(key.w + (int64_t)c * I + i0);
  double ab = 0.0;  // db of the block: three threads, so the chain can afford double and rounds once per record
  const int64_t t0 = (int64_t)blockIdx.x * tpb, t1 = t0 + tpb < tiles ? t0 + tpb : tiles;
  for (int64_t t = t0; t < t1; t++) {
    const int64_t row0 = t * 64;
    {  // stage: thread (r, c) = (tid / 4, tid % 4); c == 3 writes the flag
      const int r = tid >> 2, c = tid & 3;
      const int64_t row = row0 + r;
      const bool has = row < N && (!group || group[row] >= 0);
      float v = 0.0f;
      if (c == 3) {
        v = has ? 1.0f : 0.0f;
      } else if (has && c < nc) {
        const float p = pre[row * kHeadPreFloats + head_pre_at(kind) + c];
        float d = dp ? dp[row * dps + head_p14_at(kind) + c] : key.dout[row * key.dout_stride + c];
        if (kind == GCM_SCALE) {
          if (dp) d = d * scales[row * ss + c];
          v = (p >= -1.0f && p <= 1.0f) ? d * key.factor : 0.0f;
        } else {
          const double sg = 1.0 / (1.0 + exp(-(double)p));
          v = (float)((double)d * ((double)key.factor * sg * (1.0 - sg)));
        }
      }
      reinterpret_cast<float*>(&dvs[r])[c] = v;
    }
    __syncthreads();
    if (want_b && tid < nc)
      for (int r = 0; r < 64; r++) ab += (double)reinterpret_cast<const float*>(&dvs[r])[tid];
    if (cols && (dh || want_w)) {
      for (int r0 = 32 * rh; r0 < 32 * rh + 32; r0 += 8) {
        if (row0 + r0 >= N) break;
        f4 hv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int64_t row = row0 + r0 + u < N ? row0 + r0 + u : N - 1;  // a row beyond N has flag 0: loaded, not used
          hv[u] = want_w ? ld4(h + row * key.h_stride + i0) : zero4();
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int64_t row = row0 + r0 + u;
          const f4 d = dvs[r0 + u];
          if (row < N && dh) {
            f4 o = zero4();
            if (d[3] != 0.0f) {
              o = w[0] * d[0];
              if (nc == 3) o = o + w[1] * d[1] + w[2] * d[2];
            }
            st4(dh + row * key.dh_stride + i0, o);
          }
          if (want_w && d[3] != 0.0f) {
            aw[0] = aw[0] + hv[u] * d[0];
            if (nc == 3) {
              aw[1] = aw[1] + hv[u] * d[1];
              aw[2] = aw[2] + hv[u] * d[2];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  float* __restrict__ rec = records + (int64_t)blockIdx.y * key_floats + (int64_t)blockIdx.x * rec_floats;
  if (want_w) {
    if (rh == 1 && cols)
#pragma unroll
      for (int c = 0; c < 3; c++) half1[c][ct] = aw[c];
    __syncthreads();
    if (rh == 0 && cols)
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (c < nc) st4(rec + (int64_t)c * I + i0, aw[c] + half1[c][ct]);
  }
  if (want_b && tid < nc) rec[(int64_t)nc * I + tid] = (float)ab;
}

// ---- backward, fold ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_train_fold(const HeadKeys keys, int I, int64_t nrec, int64_t per, int groups,
                                                         int64_t rec_floats, int64_t key_floats,
                                                         const float* __restrict__ records) {
  __shared__ double part[kHeadFoldGroups][16];  // the fold adds in double and rounds once: its order costs nothing
  const gcm_head_key& key = keys.k[blockIdx.y];
  const int nc = head_channels(key.kind);
  const int64_t nw = (int64_t)nc * I, e = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const int s = threadIdx.x >> 4;
  const bool mine = e < nw + nc && (e < nw ? key.dw != nullptr : key.db != nullptr);
  if (mine && s < groups) {
    const float* __restrict__ src = records + (int64_t)blockIdx.y * key_floats + e;
    const int64_t a = (int64_t)s * per, b = a + per < nrec ? a + per : nrec;
    double v = 0.0;
    for (int64_t r = a; r < b; r++) v += (double)src[r * rec_floats];
    part[s][threadIdx.x & 15] = v;
  }
  __syncthreads();
  if (!mine || s != 0) return;
  double v = part[0][threadIdx.x];
  for (int g = 1; g < groups; g++) v += part[g][threadIdx.x];
  if (e < nw) key.dw[e] = (float)v;
  else key.db[e - nw] = (float)v;
}

// ---- host: the plan ---------------------------------------------------------------------------------------------------
struct HeadTrainPlan {
  int64_t tiles;       // tiles of 64 rows
  int64_t tpb;         // tiles a row block walks
  int64_t records;     // row blocks = records per key
  int64_t groups;      // first-level groups of the fold
  int64_t per;         // records per group
  int64_t levels;      // 1: one group, 2: groups, then the groups
  int64_t rec_floats;  // floats between records
  int64_t key_floats;  // floats between the keys' blocks of records
};
HeadTrainPlan head_train_plan(int64_t N, int32_t I) {
  HeadTrainPlan p;
  p.tiles = (N + 63) / 64;
  p.tpb = std::max<int64_t>(1, (p.tiles + kHeadMaxRecords - 1) / kHeadMaxRecords);
  p.records = (p.tiles + p.tpb - 1) / p.tpb;
  p.per = std::max<int64_t>(1, (p.records + kHeadFoldGroups - 1) / kHeadFoldGroups);
  p.groups = std::max<int64_t>(1, (p.records + p.per - 1) / p.per);
  p.levels = p.groups > 1 ? 2 : 1;
  p.rec_floats = 3 * (int64_t)I + 4;
  p.key_floats = (p.records * p.rec_floats + 63) / 64 * 64;
  return p;
}

}  // namespace
