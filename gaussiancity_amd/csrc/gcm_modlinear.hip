// gcm_modlinear.hip -- MI355X (gfx950) kernels + C ABI (include/gcm.h) of the generator's attribute head: the grouped
// modulated linear layer y = act((x o alpha[g]) W^T + beta[g] + bias), its deterministic backward, the group vector
// from the instances' masks and the head's output transform.  DESIGN.md section 17.
//
// The three products (forward, dX = dpre W, dW = dpre^T xa) run on v_mfma_f32_16x16x4_f32 with the float32 tiles of
// gcs_mfma.h: a 64 x 64 workgroup tile, 4 waves as 2 x 2, a wave owns 32 x 32 outputs = 2 x 2 accumulators of 4 VGPRs
// (C/D: col = lane & 15, row = 4 * (lane >> 4) + reg), slices of 16 along the summed index staged in LDS, the global
// loads of slice c + 1 issued before the MFMAs of slice c.  What differs from a plain GEMM is on the way in and out:
//   forward   A = x o alpha[group[row]] (one fp32 product per element, rows of one tile may be of different groups);
//             the epilogue adds beta[group[row]], then bias, applies LeakyReLU, and stores 0 for a row without a group.
//   dX        A = dpre = dy o (y > 0 ? 1 : slope), 0 for a row without a group; the epilogue stores
//             dx = dxs o alpha[group[row]] and, for dalpha, t = dxs o x into the workspace.
//   dW        both operands are staged pair(row)-major; row slices, each a chain from 0 over its rows in order, then a
//             fold over the slices in slice order (k_subm_dw_mfma's scheme).
// I, O are multiples of 4 and strides multiples of 4 elements, so every staged element is a 16-byte load that lies
// wholly inside or wholly outside its row; rows beyond N, channels beyond I / O and rows without a group are staged as
// zeros: nothing assumes a multiple of 16 or 64.
//
// The per-group sums (dalpha, dbeta; dbias from them) are kernels of this library and use no float atomics: a stable
// counting sort of the rows by group (per 256-row block a count per group, one exclusive scan over (group, block),
// then each row's rank inside its block) gives `perm`, the rows in group order and ascending inside a group; the sum
// of a group is S slices of its rows, each one chain in that order, folded in slice order.
//
// The library's second row-wise MLP, the feed-forward third of a PTv3 Block (gcm_ffn_* in one launch per direction up to 128
// channels, gcm_ffn_split_* with the hidden width split across workgroups up to 512), has its kernels and its one plan in
// gcm_ffn.h, included below; its C ABI functions are at the end of this file, thin wrappers over one argument check of the
// forward (check_ffn_forward) and one backward (ffn_backward).  DESIGN.md sections 18 and 18a.  The third, the front of the same
// Block (gcm_front_*: the convolution's Linear and LayerNorm, the residual, norm1 and the qkv projection), is gcm_front.h,
// included after it.  DESIGN.md section 19.  The fourth, the middle of the same Block around its attention (gcm_mid_*: the
// patch gather, and the scatter back, the output projection, DropPath and the residual in one launch), is gcm_mid.h.
// DESIGN.md section 20.  The fifth, the seams between the backbone's stages (gcm_seam_*: Linear, BatchNorm1d and GELU as
// one operator up to 512 channels), is gcm_seam.h.  DESIGN.md section 21.  The sixth is the attribute head itself at
// inference, its three layers in one launch per output key (gcm_head_chain), gcm_chain.h, included last.  DESIGN.md
// section 17b.  The seventh is the head's output layers in a training step, forward and backward for up to four keys
// (gcm_head_train_*), gcm_head.h.  DESIGN.md section 17c.
// What the five share -- the 64-row tile, the product loop of the four fused operators, the host rules of the plans -- is
// gcm_tile.h, included first.  DESIGN.md section 17a.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>

#include "../../include/gcm.h"
#define GC_ERR_HIP GCM_ERR_HIP
#include "gc_host.h"
#include "gcm_tile.h"

namespace {

constexpr int kSortRows = 256;    // rows per block of the counting sort
constexpr int64_t kMaxRows = (int64_t)1 << 31;
constexpr int kMaxFeatures = 65536;
constexpr int kMaxGroups = 1 << 20;

// group of a row: 0 without a group vector, -1 for a value outside 0 .. G-1
__device__ __forceinline__ int32_t row_group(const int32_t* __restrict__ group, int64_t r, int G) {
  if (!group) return 0;
  const int32_t g = group[r];
  return (g >= 0 && g < G) ? g : -1;
}

// dy o (y > 0 ? 1 : slope), four elements
__device__ __forceinline__ f4 dpre4(f4 dy, f4 y, float slope) {
  f4 r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = y[k] > 0.0f ? dy[k] : dy[k] * slope;
  return r;
}

// ---- forward and dX -------------------------------------------------------------------------------------------------
// BWD == false: out rows = x rows, summed index = I, B[k = i][col = o] = w[o][i] (read along i: Bs[col][k], kPitch).
// BWD == true:  A = dpre, summed index = O, B[k = o][col = i] = w[o][i] (read along i: Bs[k][col], kPitchT).
// K: length of the summed index, C: columns of the output.
template <bool BWD>
__global__ __launch_bounds__(256) void k_modlinear_gemm(const float* __restrict__ x, int64_t xs, const float* __restrict__ yy,
                                                        int64_t ys, const float* __restrict__ dy, int64_t dys,
                                                        const float* __restrict__ w, int64_t ws,
                                                        const float* __restrict__ alpha, const float* __restrict__ beta,
                                                        const float* __restrict__ bias, const int32_t* __restrict__ group,
                                                        int64_t N, int I, int O, int G, float slope, float* __restrict__ out,
                                                        int64_t outs, float* __restrict__ t) {
  __shared__ __attribute__((aligned(16))) float As[T * kPitch];
  __shared__ __attribute__((aligned(16))) float Bs[BWD ? KC * kPitchT : T * kPitch];
  __shared__ int32_t sG[T];
  const int tid = threadIdx.x;
  const WaveTile g;
  const int64_t row0 = (int64_t)blockIdx.x * T;
  const int n0 = blockIdx.y * T;
  const int K = BWD ? O : I, C = BWD ? I : O;
  if (tid < T) sG[tid] = row0 + tid < N ? row_group(group, row0 + tid, G) : -1;
  __syncthreads();

  // staging: A -- row tid / 4, four summed-index elements at 4 * (tid % 4); B forward the same of w's row n0 + tid / 4,
  // B dX -- summed-index row tid / 16, four columns at 4 * (tid % 16)
  const int ar = tid >> 2, ac = 4 * (tid & 3);
  const int ga = sG[ar];
  const int64_t arow = row0 + ar;
  const int br = BWD ? tid >> 4 : tid >> 2, bc = BWD ? 4 * (tid & 15) : 4 * (tid & 3);
  f4 va, vb;
  auto fetch = [&](int c0) {
    va = zero4();
    vb = zero4();
    const int c = c0 + ac;
    if (ga >= 0 && c < K) {
      if (BWD) {
        va = dpre4(ld4(dy + arow * dys + c), ld4(yy + arow * ys + c), slope);
      } else {
        va = ld4(x + arow * xs + c);
        if (alpha) va = va * ld4(alpha + (int64_t)ga * I + c);
      }
    }
    if (BWD) {
      const int o = c0 + br, i = n0 + bc;
      if (o < O && i < I) vb = ld4(w + (int64_t)o * ws + i);
    } else {
      const int o = n0 + br, i = c0 + bc;
      if (o < O && i < I) vb = ld4(w + (int64_t)o * ws + i);
    }
  };

  f4 acc[2][2];
  clear_acc(acc);
  fetch(0);
  for (int c0 = 0; c0 < K; c0 += KC) {
    *reinterpret_cast<f4*>(&As[ar * kPitch + ac]) = va;
    *reinterpret_cast<f4*>(&Bs[BWD ? br * kPitchT + bc : br * kPitch + bc]) = vb;
    __syncthreads();
    if (c0 + KC < K) fetch(c0 + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) a[i] = As[(g.wr + 16 * i + g.fl) * kPitch + kk + g.fk];
#pragma unroll
      for (int j = 0; j < 2; j++)
        b[j] = BWD ? Bs[(kk + g.fk) * kPitchT + g.wc + 16 * j + g.fl] : Bs[(g.wc + 16 * j + g.fl) * kPitch + kk + g.fk];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int rl = g.wr + 16 * i + 4 * g.fk + v;
      const int64_t row = row0 + rl;
      if (row >= N) continue;
      const int gr = sG[rl];
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int c = n0 + g.wc + 16 * j + g.fl;
        if (c >= C) continue;
        float val = acc[i][j][v];
        if (BWD) {
          if (t) t[row * I + c] = gr >= 0 ? val * x[row * xs + c] : 0.0f;
          if (out) out[row * outs + c] = gr >= 0 ? (alpha ? val * alpha[(int64_t)gr * I + c] : val) : 0.0f;
        } else {
          if (beta && gr >= 0) val += beta[(int64_t)gr * O + c];
          if (bias) val += bias[c];
          val = val > 0.0f ? val : val * slope;
          out[row * outs + c] = gr >= 0 ? val : 0.0f;
        }
      }
    }
}

// ---- dW -------------------------------------------------------------------------------------------------------------
// part[s][o][i] (or dw itself with one slice) = sum over the rows r of slice s, ascending, of dpre[r][o] * xa[r][i].
// Pair-major images Ds[pair][o] and Xs[pair][i] at kPitchT; a thread stages pair tid / 16, four columns at 4 * (tid % 16).
__global__ __launch_bounds__(256) void k_modlinear_dw(const float* __restrict__ x, int64_t xs, const float* __restrict__ yy,
                                                      int64_t ys, const float* __restrict__ dy, int64_t dys,
                                                      const float* __restrict__ alpha, const int32_t* __restrict__ group,
                                                      int64_t N, int I, int O, int G, float slope, int64_t per,
                                                      float* __restrict__ part, float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float Ds[KC * kPitchT];
  __shared__ __attribute__((aligned(16))) float Xs[KC * kPitchT];
  const int tid = threadIdx.x;
  const WaveTile g;
  const int tiles_i = (I + T - 1) / T;
  const int o0 = (blockIdx.x / tiles_i) * T, i0 = (blockIdx.x % tiles_i) * T;
  const int s = blockIdx.y;
  const int64_t p0 = s * per, p1 = p0 + per < N ? p0 + per : N;
  const int sp = tid >> 4, sc = 4 * (tid & 15);
  f4 vd, vx;
  auto fetch = [&](int64_t p) {
    vd = zero4();
    vx = zero4();
    const int64_t r = p + sp;
    if (r >= p1) return;
    const int gr = row_group(group, r, G);
    if (gr < 0) return;
    if (o0 + sc < O) vd = dpre4(ld4(dy + r * dys + o0 + sc), ld4(yy + r * ys + o0 + sc), slope);
    if (i0 + sc < I) {
      vx = ld4(x + r * xs + i0 + sc);
      if (alpha) vx = vx * ld4(alpha + (int64_t)gr * I + i0 + sc);
    }
  };
  f4 acc[2][2];
  clear_acc(acc);
  fetch(p0);
  for (int64_t p = p0; p < p1; p += KC) {
    *reinterpret_cast<f4*>(&Ds[sp * kPitchT + sc]) = vd;
    *reinterpret_cast<f4*>(&Xs[sp * kPitchT + sc]) = vx;
    __syncthreads();
    if (p + KC < p1) fetch(p + KC);
#pragma unroll
    for (int kk = 0; kk < KC; kk += 4) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) a[i] = Ds[(kk + g.fk) * kPitchT + g.wr + 16 * i + g.fl];
#pragma unroll
      for (int j = 0; j < 2; j++) b[j] = Xs[(kk + g.fk) * kPitchT + g.wc + 16 * j + g.fl];
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  float* dst = part ? part + (int64_t)s * O * I : dw;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int o = o0 + g.wr + 16 * i + 4 * g.fk + v;
      if (o >= O) continue;
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int c = i0 + g.wc + 16 * j + g.fl;
        if (c < I) dst[(int64_t)o * I + c] = acc[i][j][v];
      }
    }
}

// out[e] = sum of part[s][e], s ascending
__global__ void k_fold_slices(const float* __restrict__ part, int S, int64_t len, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= len) return;
  float v = part[e];
  for (int s = 1; s < S; s++) v += part[(int64_t)s * len + e];
  out[e] = v;
}

// ---- rows in group order --------------------------------------------------------------------------------------------
// cnt[g][b]: rows of group g in block b (every entry is written)
__global__ __launch_bounds__(kSortRows) void k_sort_count(const int32_t* __restrict__ group, int64_t N, int G, int64_t NB,
                                                          int32_t* __restrict__ cnt) {
  __shared__ int32_t sg[kSortRows];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kSortRows + tid;
  sg[tid] = r < N ? row_group(group, r, G) : -1;
  __syncthreads();
  for (int gq = tid; gq < G; gq += kSortRows) {
    int32_t c = 0;
    for (int j = 0; j < kSortRows; j++) c += sg[j] == gq;
    cnt[(int64_t)gq * NB + blockIdx.x] = c;
  }
}

// exclusive scan of cnt in place (one workgroup: every thread a contiguous run), start[g] = first position of group g,
// start[G] = the number of rows that have a group
__global__ __launch_bounds__(1024) void k_sort_scan(int32_t* __restrict__ cnt, int64_t len, int G, int64_t NB,
                                                    int32_t* __restrict__ start) {
  __shared__ int32_t sums[1024];
  const int tid = threadIdx.x;
  const int64_t run = (len + 1023) / 1024;
  const int64_t e0 = tid * run, e1 = e0 + run < len ? e0 + run : len;
  int32_t sum = 0;
  for (int64_t e = e0; e < e1; e++) sum += cnt[e];
  sums[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int32_t acc = 0;
    for (int k = 0; k < 1024; k++) {
      const int32_t v = sums[k];
      sums[k] = acc;
      acc += v;
    }
    start[G] = acc;
  }
  __syncthreads();
  int32_t acc = sums[tid];
  for (int64_t e = e0; e < e1; e++) {
    const int32_t v = cnt[e];
    cnt[e] = acc;
    if (e % NB == 0) start[e / NB] = acc;
    acc += v;
  }
}

// perm[first position of (group, block) + rank of the row among the block's rows of its group] = row
__global__ __launch_bounds__(kSortRows) void k_sort_place(const int32_t* __restrict__ group, int64_t N, int G, int64_t NB,
                                                          const int32_t* __restrict__ first, int32_t* __restrict__ perm) {
  __shared__ int32_t sg[kSortRows];
  const int tid = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kSortRows + tid;
  const int32_t gr = r < N ? row_group(group, r, G) : -1;
  sg[tid] = gr;
  __syncthreads();
  if (gr < 0) return;
  int32_t rank = 0;
  for (int j = 0; j < tid; j++) rank += sg[j] == gr;
  perm[first[(int64_t)gr * NB + blockIdx.x] + rank] = (int32_t)r;
}

// gpart[s][g][col], col < I: sum of t[r][col]; col >= I: sum of dpre[r][col - I] -- over the rows of slice s of group g,
// in perm's order.  grid.x = G * column blocks, grid.y = S.  Without perm (no group vector) the rows are 0 .. N-1.
__global__ __launch_bounds__(256) void k_group_sum(const float* __restrict__ t, const float* __restrict__ yy, int64_t ys,
                                                   const float* __restrict__ dy, int64_t dys,
                                                   const int32_t* __restrict__ perm, const int32_t* __restrict__ start,
                                                   int64_t N, int I, int O, int G, int S, float slope,
                                                   float* __restrict__ gpart) {
  const int C = I + O, cblocks = (C + 255) / 256;
  const int gq = blockIdx.x / cblocks, col = (blockIdx.x % cblocks) * 256 + threadIdx.x, s = blockIdx.y;
  if (col >= C) return;
  const int64_t b0 = start ? start[gq] : 0, b1 = start ? start[gq + 1] : (gq == 0 ? N : 0);
  const int64_t per = (b1 - b0 + S - 1) / S;
  const int64_t p0 = b0 + s * per, p1 = p0 + per < b1 ? p0 + per : b1;
  auto term = [&](int64_t p) {
    const int64_t r = perm ? perm[p] : p;
    if (col < I) return t ? t[r * I + col] : 0.0f;
    const int o = col - I;
    const float d = dy[r * dys + o];
    return yy[r * ys + o] > 0.0f ? d : d * slope;
  };
  float acc = 0.0f;
  int64_t p = p0;
  for (; p + 4 <= p1; p += 4) {  // four rows' loads in flight; the sum stays one chain in row order
    const float v0 = term(p), v1 = term(p + 1), v2 = term(p + 2), v3 = term(p + 3);
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; p < p1; p++) acc += term(p);
  gpart[((int64_t)s * G + gq) * C + col] = acc;
}

// dalpha[g][i], dbeta[g][o]: the slices of gpart in slice order; dbias[o]: the groups in ascending order, each its slices
__global__ void k_group_fold(const float* __restrict__ gpart, int S, int G, int I, int O, float* __restrict__ dalpha,
                             float* __restrict__ dbeta, float* __restrict__ dbias) {
  const int C = I + O;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, per_group = (int64_t)G * C;
  if (e < per_group) {
    const int gq = (int)(e / C), col = (int)(e % C);
    float v = gpart[e];
    for (int s = 1; s < S; s++) v += gpart[(int64_t)s * per_group + e];
    if (col < I) {
      if (dalpha) dalpha[(int64_t)gq * I + col] = v;
    } else if (dbeta) {
      dbeta[(int64_t)gq * O + col - I] = v;
    }
  } else if (e < per_group + O && dbias) {
    const int o = (int)(e - per_group);
    float total = 0.0f;
    for (int gq = 0; gq < G; gq++) {
      float v = gpart[(int64_t)gq * C + I + o];
      for (int s = 1; s < S; s++) v += gpart[(int64_t)s * per_group + (int64_t)gq * C + I + o];
      total += v;
    }
    dbias[o] = total;
  }
}

// ---- group vector from the instances' masks ---------------------------------------------------------------------------
__global__ void k_groups_from_masks(const uint8_t* const* __restrict__ masks, int G, int64_t N, int32_t* __restrict__ group) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  int32_t found = -1;
  for (int gq = G - 1; gq >= 0; gq--)
    if (masks[gq][r]) {
      found = gq;
      break;
    }
  group[r] = found;
}

// ---- output transform of the head -------------------------------------------------------------------------------------
// 16 lanes per row: lane q sums the elements 4 q + 64 k .. + 3 (k ascending), then a fixed exchange tree over the 16.
template <int NC>
__global__ __launch_bounds__(256) void k_head_out(const float* __restrict__ f, int64_t fs, const float* __restrict__ w,
                                                  const float* __restrict__ b, const int32_t* __restrict__ group, int64_t N,
                                                  int I, int kind, float factor, float* __restrict__ out) {
  const int q = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = row < N;
  const int gr = !live ? -1 : (group ? (group[row] >= 0 ? 0 : -1) : 0);  // here only "has a group" matters
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) acc[c] = 0.0f;
  if (gr >= 0) {
    for (int i = 4 * q; i < I; i += 64) {
      const f4 v = ld4(f + row * fs + i);
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const f4 wv = ld4(w + (int64_t)c * I + i);
#pragma unroll
        for (int k = 0; k < 4; k++) acc[c] += v[k] * wv[k];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; c++)
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) acc[c] += __shfl_xor(acc[c], m, 64);
  if (!live || q != 0) return;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    float res = 0.0f;
    if (gr >= 0) {
      const float v = b ? acc[c] + b[c] : acc[c];
      const double sg = 1.0 / (1.0 + exp(-(double)v));
      double d;
      if (kind == GCM_SCALE) d = 1.0 + (double)fminf(fmaxf(v, -1.0f), 1.0f) * (double)factor;
      else if (kind == GCM_OPACITY) d = sg * (double)factor + (1.0 - (double)factor);
      else d = (sg - 0.5) * (double)factor;
      res = (float)d;
    }
    out[row * NC + c] = res;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool stride_ok(int64_t s, int width) { return s > 0 && s % 4 == 0 && s >= width; }
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// The checks every entry point repeats, each with the one message it has always had.
struct Stride {
  int64_t s;
  int width;
  bool used = true;  // false: the tensor it belongs to was not passed
};
int check_strides(const std::string& w, std::initializer_list<Stride> strides) {
  for (const Stride& x : strides)
    if (x.used && !stride_ok(x.s, x.width))
      return fail(GCM_ERR_INVALID_ARGUMENT, w + ": strides must be positive multiples of 4 elements, at least the row's width");
  return 0;
}
int check_aligned16(const std::string& w, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!aligned16(p)) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": float pointers must be 16-byte aligned");
  return 0;
}
int check_workspace(const std::string& w, const void* workspace, size_t bytes, size_t need, const char* sizer) {
  if (bytes < need || !workspace) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": workspace smaller than " + sizer);
  if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0)
    return fail(GCM_ERR_INVALID_ARGUMENT, w + ": workspace must be 256-byte aligned");
  return 0;
}
// N == 0: the outputs that are sums over the rows are zeros; a null output is skipped
struct Clear {
  void* p;
  size_t bytes;
  const char* what;
};
int clear_outputs(hipStream_t st, std::initializer_list<Clear> outs) {
  for (const Clear& c : outs)
    if (c.p) HIP_TRY(hipMemsetAsync(c.p, 0, c.bytes, st), c.what);
  return GCM_OK;
}

int check_shape(const std::string& w, int64_t N, int32_t I, int32_t O, int32_t G) {
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (I <= 0 || I % 4 != 0 || I > kMaxFeatures) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": I must be a positive multiple of 4");
  if (O <= 0 || O % 4 != 0 || O > kMaxFeatures) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": O must be a positive multiple of 4");
  if (G < 1 || G > kMaxGroups) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": G must be in 1..2^20");
  return 0;
}
// the backward's counting sort keeps one count per (group, block of 256 rows)
int check_sort(const std::string& w, int64_t N, int32_t G) {
  if (((N + kSortRows - 1) / kSortRows) * (int64_t)G >= kMaxRows)
    return fail(GCM_ERR_INVALID_ARGUMENT, w + ": ceil(N / 256) * G does not fit 31 bits");
  return 0;
}

// The backward's slices and the carve of its workspace (offsets in bytes, each a multiple of 256).
struct BackwardPlan {
  int sw;      // row slices of dW
  int sg;      // slices of a group's rows
  int64_t nb;  // blocks of the counting sort
  size_t t, wpart, cnt, start, perm, gpart, total;
};
BackwardPlan plan_backward(int64_t N, int32_t I, int32_t O, int32_t G) {
  BackwardPlan p;
  const int64_t tiles = (int64_t)((O + T - 1) / T) * ((I + T - 1) / T);
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(64, 1024 / tiles));
  p.sw = (int)std::max<int64_t>(1, std::min<int64_t>(cap, (N + 127) / 128));
  p.sg = (int)std::max<int64_t>(1, std::min<int64_t>(256, (N + 64 * (int64_t)G - 1) / (64 * (int64_t)G)));
  p.nb = (N + kSortRows - 1) / kSortRows;
  Carve ws;
  p.t = ws.take((size_t)N * I * 4);
  p.wpart = ws.take(p.sw > 1 ? (size_t)p.sw * O * I * 4 : 0);
  p.cnt = ws.take((size_t)p.nb * G * 4);
  p.start = ws.take(((size_t)G + 1) * 4);
  p.perm = ws.take((size_t)N * 4);
  p.gpart = ws.take((size_t)p.sg * G * ((size_t)I + O) * 4);
  p.total = ws.off;
  return p;
}

}  // namespace

#include "gcm_ffn.h"
#include "gcm_front.h"
#include "gcm_mid.h"
#include "gcm_seam.h"
#include "gcm_chain.h"
#include "gcm_head.h"

namespace {

// split: the gcm_ffn_split_* entry points, whose cap is their own
int check_ffn_shape(const std::string& w, bool split, int64_t N, int32_t C, int32_t Hd) {
  const int cap = split ? kFfnSplitMaxChannels : kFfnMaxChannels;
  const std::string query = split ? "gcm_ffn_split_max_channels()" : "gcm_ffn_max_channels()";
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (C <= 0 || C % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C must be a positive multiple of 4");
  if (Hd <= 0 || Hd % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": Hd must be a positive multiple of 4");
  if (C > cap) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C above " + query);
  if (Hd > 4 * cap) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": Hd above 4 * " + query);
  return 0;
}

// The arguments of either forward entry point, and the plan.  The split one has a workspace: the partial records.  After
// a 0 the caller returns at once when N == 0 -- the pointers are looked at for N > 0 only.
int check_ffn_forward(const std::string& who, bool split, const float* x, int64_t x_stride, const float* ln_w, const float* ln_b,
                      float eps, const float* w1, const float* b1, const float* w2, const float* b2, int64_t N, int32_t C,
                      int32_t Hd, const float* y, int64_t y_stride, const float* mean, const float* rstd, const float* a,
                      const void* workspace, size_t workspace_bytes, FfnPlan& p) {
  if (int rc = check_ffn_shape(who, split, N, C, Hd)) return rc;
  if (!std::isfinite(eps) || eps < 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": eps must be finite and >= 0");
  if (int rc = check_strides(who, {{x_stride, C}, {y_stride, C}})) return rc;
  if (int rc = check_aligned16(who, {x, ln_w, ln_b, w1, b1, w2, b2, y, a})) return rc;
  p = ffn_plan(N, C, Hd, split);
  if (split)
    if (int rc = check_workspace(who, workspace, workspace_bytes, std::max<size_t>(p.fwd_total, 256), "gcm_ffn_split_workspace_bytes"))
      return rc;
  if (N == 0) return 0;
  if (!x || !ln_w || !ln_b || !w1 || !b1 || !w2 || !b2 || !y)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, ln_w, ln_b, w1, b1, w2, b2 or y");
  if ((mean == nullptr) != (rstd == nullptr) || (a && !mean))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": mean and rstd come together, and a needs both");
  return 0;
}

// Either backward entry point.  split chooses the plan, the workspace query the message names, the row-side launches -- one
// kernel, or partial records and the kernel that folds them -- and the prefix of the HIP error labels; the checks, the N == 0
// clears, the gating of the launches, the LayerNorm fold and the weight-gradient half are the same.
int ffn_backward(const std::string& who, bool split, const float* x, int64_t x_stride, const float* mean, const float* rstd,
                 const float* a, const float* dy, int64_t dy_stride, const float* row_scale, const float* ln_w, const float* ln_b,
                 const float* w1, const float* w2, int64_t N, int32_t C, int32_t Hd, float* dx, int64_t dx_stride, float* dln_w,
                 float* dln_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes,
                 void* hip_stream) {
  const std::string label = split ? "ffn split backward " : "ffn backward ";
  auto at = [&](const char* what) { return label + what; };
  if (int rc = check_ffn_shape(who, split, N, C, Hd)) return rc;
  if (int rc = check_strides(who, {{x_stride, C}, {dy_stride, C}, {dx_stride, C, dx != nullptr}})) return rc;
  if (int rc = check_aligned16(who, {x, a, dy, ln_w, ln_b, w1, w2, dx, dln_w, dln_b, dw1, db1, dw2, db2})) return rc;
  const FfnPlan p = ffn_plan(N, C, Hd, split);
  if (int rc = check_workspace(who, workspace, workspace_bytes, p.total,
                               split ? "gcm_ffn_split_workspace_bytes" : "gcm_ffn_backward_workspace_bytes"))
    return rc;
  if (N > 0 && (!x || !mean || !rstd || !a || !dy || !ln_w || !ln_b || !w1 || !w2))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, mean, rstd, a, dy, ln_w, ln_b, w1 or w2");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0) {  // nothing to sum: the parameter gradients are zeros
    const size_t CH = (size_t)C * Hd * 4, C4 = (size_t)C * 4;
    return clear_outputs(st, {{dln_w, C4, at("clear dln_w").c_str()},  // the labels live to the end of this statement
                              {dln_b, C4, at("clear dln_b").c_str()},
                              {dw1, CH, at("clear dw1").c_str()},
                              {db1, (size_t)Hd * 4, at("clear db1").c_str()},
                              {dw2, CH, at("clear dw2").c_str()},
                              {db2, C4, at("clear db2").c_str()}});
  }
  if (split) HIP_TRY(split_lds_attr(), "ffn split LDS attribute");
  char* ws = (char*)workspace;
  float* da = (float*)(ws + p.da);
  const bool ln = dln_w || dln_b, first = dw1 || db1, params = first || dw2 || db2;
  if (dx || ln || first) {
    float* lnpart = ln ? (float*)(ws + p.lnpart) : nullptr;
    if (!split) {
      with_nj(C, [&](auto nj) {
        k_ffn_bwd_rows<decltype(nj)::value><<<(unsigned)p.tiles, 256, 0, st>>>(x, x_stride, mean, rstd, a, dy, dy_stride, row_scale,
                                                                              ln_w, w1, w2, N, C, Hd, dx, dx_stride, da, lnpart);
      });
    } else {
      float* part = (float*)(ws + p.part);
      with_split_width(C, [&](auto nj, auto nb) {
        constexpr int NJ = decltype(nj)::value, NB = decltype(nb)::value;
        const dim3 grid((unsigned)p.tiles, (unsigned)p.records);
        if (p.split)
          k_ffn_split_bwd_rows<NJ, NB, true><<<grid, 256, split_bwd_lds(NJ, NB), st>>>(a, dy, dy_stride, row_scale, w1, w2, N, C, Hd, da,
                                                                                       part);
        else
          k_ffn_split_bwd_rows<NJ, NB, false><<<grid, 256, split_bwd_lds(NJ, NB), st>>>(a, dy, dy_stride, row_scale, w1, w2, N, C, Hd, da,
                                                                                        part);
        if (dx || ln)
          k_ffn_split_bwd_ln<NJ, NB><<<(unsigned)p.tiles, 256, split_ln_lds(NJ, NB), st>>>(
              part, (int)p.records, x, x_stride, mean, rstd, dy, dy_stride, ln_w, N, C, dx, dx_stride, lnpart);
      });
    }
    HIP_TRY(hipGetLastError(), at("rows launch").c_str());
    if (ln) {
      fold_ln_partials(lnpart, (float*)(ws + p.lngroup), p.tiles, p.groups, p.gper, 2, C, dln_w, dln_b, nullptr, nullptr, st);
      HIP_TRY(hipGetLastError(), at("LayerNorm fold launch").c_str());
    }
  }
  if (params) {
    const int64_t per = slice_rows(N, p.sw);
    float* wpart = (float*)(ws + p.wpart);
    const dim3 grid(blocks_for(Hd, T) * blocks_for(C, T), (unsigned)p.sw, 2);
    k_ffn_dw<<<grid, 256, 0, st>>>(x, x_stride, mean, rstd, a, da, dy, dy_stride, row_scale, ln_w, ln_b, N, (int)C, (int)Hd, per,
                                   wpart);
    k_ffn_fold_params<<<blocks_for(ffn_record(C, Hd), 256), 256, 0, st>>>(wpart, p.sw, (int64_t)C * Hd, (int64_t)C * Hd, Hd, C, dw1,
                                                                          dw2, db1, db2);
    HIP_TRY(hipGetLastError(), at("weight gradient launch").c_str());
  }
  return GCM_OK;
}

int check_front_shape(const std::string& w, int64_t N, int32_t C, int32_t O) {
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (C <= 0 || C % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C must be a positive multiple of 4");
  if (O <= 0 || O % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": O must be a positive multiple of 4");
  if (C > kFrontMaxChannels) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C above gcm_front_max_channels()");
  if (O > 3 * kFrontMaxChannels) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": O above 3 * gcm_front_max_channels()");
  return 0;
}

int check_mid_shape(const std::string& w, int64_t N, int32_t C) {
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (C <= 0 || C % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C must be a positive multiple of 4");
  if (C > kMidMaxChannels) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": C above gcm_mid_max_channels()");
  return 0;
}
// rows of W floats copied in 16-byte pieces, one thread a piece
int check_mid_width(const std::string& w, int64_t rows, int32_t W) {
  if (W <= 0 || W % 4 != 0 || W > kMaxFeatures) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": W must be a positive multiple of 4");
  if ((rows * (W / 4) + 255) / 256 >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": rows * W / 4 does not fit 39 bits");
  return 0;
}
int check_seam_shape(const std::string& w, int64_t N, int32_t I, int32_t O, bool product) {
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (I <= 0 || I % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": I must be a positive multiple of 4");
  if (O <= 0 || O % 4 != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": O must be a positive multiple of 4");
  if (I > kSeamMaxChannels || O > kSeamMaxChannels)
    return fail(GCM_ERR_INVALID_ARGUMENT, w + ": I or O above gcm_seam_max_channels()");
  if (!product && I != O) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": w == NULL needs I == O");
  return 0;
}

}  // namespace

extern "C" {

int gcm_abi_version(void) { return GCM_ABI_VERSION; }
const char* gcm_last_error(void) { return g_err.c_str(); }

int gcm_groups_from_masks(const void* masks, int64_t G, int64_t N, int32_t* group, void* hip_stream) {
  const std::string w("gcm_groups_from_masks");
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (G < 0 || G > kMaxGroups) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": G must be in 0..2^20");
  if (N == 0) return GCM_OK;
  if (!group) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": null group");
  if (G > 0 && !masks) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": null masks");
  if ((reinterpret_cast<uintptr_t>(masks) & 7u) != 0) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": masks must be 8-byte aligned");
  k_groups_from_masks<<<blocks_for(N, 256), 256, 0, (hipStream_t)hip_stream>>>((const uint8_t* const*)masks, (int)G, N, group);
  HIP_TRY(hipGetLastError(), "groups_from_masks launch");
  return GCM_OK;
}

int gcm_modlinear_forward(const float* x, int64_t x_stride, const float* w, int64_t w_stride, const float* alpha,
                          const float* beta, const float* bias, const int32_t* group, int64_t N, int32_t I, int32_t O,
                          int32_t G, float slope, float* y, int64_t y_stride, void* hip_stream) {
  const std::string who("gcm_modlinear_forward");
  if (int rc = check_shape(who, N, I, O, G)) return rc;
  if (!std::isfinite(slope) || slope <= 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": slope must be finite and > 0");
  if (int rc = check_strides(who, {{x_stride, I}, {w_stride, I}, {y_stride, O}})) return rc;
  if (int rc = check_aligned16(who, {x, w, alpha, beta, bias, y})) return rc;
  if (N == 0) return GCM_OK;
  if (!x || !w || !y) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, w or y");
  const dim3 grid(blocks_for(N, T), blocks_for(O, T));
  k_modlinear_gemm<false><<<grid, 256, 0, (hipStream_t)hip_stream>>>(x, x_stride, nullptr, 0, nullptr, 0, w, w_stride, alpha,
                                                                     beta, bias, group, N, I, O, G, slope, y, y_stride,
                                                                     nullptr);
  HIP_TRY(hipGetLastError(), "modlinear forward launch");
  return GCM_OK;
}

size_t gcm_modlinear_backward_workspace_bytes(int64_t N, int32_t I, int32_t O, int32_t G) {
  if (check_shape("gcm_modlinear_backward_workspace_bytes", N, I, O, G)) return 0;
  if (check_sort("gcm_modlinear_backward_workspace_bytes", N, G)) return 0;
  g_err.clear();
  return plan_backward(N, I, O, G).total;
}

int gcm_modlinear_backward(const float* x, int64_t x_stride, const float* y, int64_t y_stride, const float* dy,
                           int64_t dy_stride, const float* w, int64_t w_stride, const float* alpha,
                           const int32_t* group, int64_t N, int32_t I, int32_t O, int32_t G, float slope, float* dx,
                           int64_t dx_stride, float* dw, float* dalpha, float* dbeta, float* dbias, void* workspace,
                           size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_modlinear_backward");
  if (int rc = check_shape(who, N, I, O, G)) return rc;
  if (int rc = check_sort(who, N, G)) return rc;
  if (!std::isfinite(slope) || slope <= 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": slope must be finite and > 0");
  if (int rc = check_strides(who, {{x_stride, I}, {y_stride, O}, {dy_stride, O}, {w_stride, I}, {dx_stride, I, dx != nullptr}}))
    return rc;
  if (int rc = check_aligned16(who, {x, y, dy, w, alpha, dx, dw, dalpha, dbeta, dbias})) return rc;
  const BackwardPlan p = plan_backward(N, I, O, G);
  if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, "gcm_modlinear_backward_workspace_bytes")) return rc;
  if (N > 0 && (!x || !y || !dy || !w)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, y, dy or w");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0)  // nothing to sum: the outputs that do not depend on N are zeros
    return clear_outputs(st, {{dw, (size_t)O * I * 4, "backward clear dw"},
                              {dalpha, (size_t)G * I * 4, "backward clear dalpha"},
                              {dbeta, (size_t)G * O * 4, "backward clear dbeta"},
                              {dbias, (size_t)O * 4, "backward clear dbias"}});
  char* ws = (char*)workspace;
  float* t = dalpha ? (float*)(ws + p.t) : nullptr;
  if (dx || t) {
    const dim3 grid(blocks_for(N, T), blocks_for(I, T));
    k_modlinear_gemm<true><<<grid, 256, 0, st>>>(x, x_stride, y, y_stride, dy, dy_stride, w, w_stride, alpha, nullptr,
                                                 nullptr, group, N, I, O, G, slope, dx, dx_stride, t);
    HIP_TRY(hipGetLastError(), "modlinear dx launch");
  }
  if (dw) {
    const int64_t per = slice_rows(N, p.sw);
    float* part = p.sw > 1 ? (float*)(ws + p.wpart) : nullptr;
    const dim3 grid(blocks_for(O, T) * blocks_for(I, T), (unsigned)p.sw);
    k_modlinear_dw<<<grid, 256, 0, st>>>(x, x_stride, y, y_stride, dy, dy_stride, alpha, group, N, I, O, G, slope, per,
                                         part, dw);
    HIP_TRY(hipGetLastError(), "modlinear dw launch");
    if (part) {
      k_fold_slices<<<blocks_for((int64_t)O * I, 256), 256, 0, st>>>(part, p.sw, (int64_t)O * I, dw);
      HIP_TRY(hipGetLastError(), "modlinear dw fold launch");
    }
  }
  if (dalpha || dbeta || dbias) {
    int32_t* perm = nullptr;
    int32_t* start = nullptr;
    if (group) {
      int32_t* cnt = (int32_t*)(ws + p.cnt);
      start = (int32_t*)(ws + p.start);
      perm = (int32_t*)(ws + p.perm);
      k_sort_count<<<(unsigned)p.nb, kSortRows, 0, st>>>(group, N, G, p.nb, cnt);
      k_sort_scan<<<1, 1024, 0, st>>>(cnt, p.nb * G, G, p.nb, start);
      k_sort_place<<<(unsigned)p.nb, kSortRows, 0, st>>>(group, N, G, p.nb, cnt, perm);
      HIP_TRY(hipGetLastError(), "modlinear sort launch");
    }
    float* gpart = (float*)(ws + p.gpart);
    const int C = I + O;
    const dim3 grid((unsigned)G * blocks_for(C, 256), (unsigned)p.sg);
    k_group_sum<<<grid, 256, 0, st>>>(t, y, y_stride, dy, dy_stride, perm, start, N, I, O, G, p.sg, slope, gpart);
    k_group_fold<<<blocks_for((int64_t)G * C + O, 256), 256, 0, st>>>(gpart, p.sg, G, I, O, dalpha, dbeta, dbias);
    HIP_TRY(hipGetLastError(), "modlinear group sums launch");
  }
  return GCM_OK;
}

int gcm_head_out(const float* f, int64_t f_stride, const float* w_out, const float* b, const int32_t* group, int64_t N,
                 int32_t I, int32_t C, int kind, float factor, float* out, void* hip_stream) {
  const std::string who("gcm_head_out");
  if (int rc = check_shape(who, N, I, 4, 1)) return rc;
  if (C != 1 && C != 3) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": C must be 1 or 3");
  if (kind != GCM_XYZ && kind != GCM_RGB && kind != GCM_SCALE && kind != GCM_OPACITY)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": unknown kind");
  if (!std::isfinite(factor)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": factor is not finite");
  if (int rc = check_strides(who, {{f_stride, I}})) return rc;
  if (int rc = check_aligned16(who, {f, w_out})) return rc;
  if (N == 0) return GCM_OK;
  if (!f || !w_out || !out) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null f, w_out or out");
  hipStream_t st = (hipStream_t)hip_stream;
  if (C == 1) k_head_out<1><<<blocks_for(N, 16), 256, 0, st>>>(f, f_stride, w_out, b, group, N, I, kind, factor, out);
  else k_head_out<3><<<blocks_for(N, 16), 256, 0, st>>>(f, f_stride, w_out, b, group, N, I, kind, factor, out);
  HIP_TRY(hipGetLastError(), "head_out launch");
  return GCM_OK;
}

int gcm_ffn_max_channels(void) { return kFfnMaxChannels; }

int gcm_ffn_forward(const float* x, int64_t x_stride, const float* ln_w, const float* ln_b, float eps, const float* w1,
                    const float* b1, const float* w2, const float* b2, const float* row_scale, int64_t N, int32_t C,
                    int32_t Hd, float* y, int64_t y_stride, float* mean, float* rstd, float* a, void* hip_stream) {
  FfnPlan p;
  if (int rc = check_ffn_forward("gcm_ffn_forward", false, x, x_stride, ln_w, ln_b, eps, w1, b1, w2, b2, N, C, Hd, y, y_stride, mean,
                                 rstd, a, nullptr, 0, p))
    return rc;
  if (N == 0) return GCM_OK;
  with_nj(C, [&](auto nj) {
    k_ffn_forward<decltype(nj)::value><<<(unsigned)p.tiles, 256, 0, (hipStream_t)hip_stream>>>(
        x, x_stride, ln_w, ln_b, eps, w1, b1, w2, b2, row_scale, N, C, Hd, y, y_stride, mean, rstd, a);
  });
  HIP_TRY(hipGetLastError(), "ffn forward launch");
  return GCM_OK;
}

size_t gcm_ffn_backward_workspace_bytes(int64_t N, int32_t C, int32_t Hd) {
  if (check_ffn_shape("gcm_ffn_backward_workspace_bytes", false, N, C, Hd)) return 0;
  g_err.clear();
  return ffn_plan(N, C, Hd, false).total;
}

int gcm_ffn_backward(const float* x, int64_t x_stride, const float* mean, const float* rstd, const float* a,
                     const float* dy, int64_t dy_stride, const float* row_scale, const float* ln_w, const float* ln_b,
                     const float* w1, const float* w2, int64_t N, int32_t C, int32_t Hd, float* dx, int64_t dx_stride,
                     float* dln_w, float* dln_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                     size_t workspace_bytes, void* hip_stream) {
  return ffn_backward("gcm_ffn_backward", false, x, x_stride, mean, rstd, a, dy, dy_stride, row_scale, ln_w, ln_b, w1, w2, N, C, Hd,
                      dx, dx_stride, dln_w, dln_b, dw1, db1, dw2, db2, workspace, workspace_bytes, hip_stream);
}

int gcm_ffn_split_max_channels(void) { return kFfnSplitMaxChannels; }

int gcm_ffn_split_plan(int64_t N, int32_t C, int32_t Hd, int64_t plan[8]) {
  const std::string who("gcm_ffn_split_plan");
  if (int rc = check_ffn_shape(who, true, N, C, Hd)) return rc;
  if (!plan) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null plan");
  const FfnPlan p = ffn_plan(N, C, Hd, true);
  const int64_t out[8] = {p.split ? 1 : 0, p.tiles, p.chunks, p.records, p.sw, p.groups, kFfnSplitLimit, 0};
  std::copy(out, out + 8, plan);
  return GCM_OK;
}

int gcm_ffn_split_workspace_bytes(int64_t N, int32_t C, int32_t Hd, size_t* forward_bytes, size_t* backward_bytes) {
  if (int rc = check_ffn_shape("gcm_ffn_split_workspace_bytes", true, N, C, Hd)) return rc;
  const FfnPlan p = ffn_plan(N, C, Hd, true);
  if (forward_bytes) *forward_bytes = std::max<size_t>(p.fwd_total, 256);  // never 0 for arguments in range
  if (backward_bytes) *backward_bytes = p.total;
  return GCM_OK;
}

int gcm_ffn_split_forward(const float* x, int64_t x_stride, const float* ln_w, const float* ln_b, float eps, const float* w1,
                          const float* b1, const float* w2, const float* b2, const float* row_scale, int64_t N, int32_t C,
                          int32_t Hd, float* y, int64_t y_stride, float* mean, float* rstd, float* a, void* workspace,
                          size_t workspace_bytes, void* hip_stream) {
  FfnPlan p;
  if (int rc = check_ffn_forward("gcm_ffn_split_forward", true, x, x_stride, ln_w, ln_b, eps, w1, b1, w2, b2, N, C, Hd, y, y_stride,
                                 mean, rstd, a, workspace, workspace_bytes, p))
    return rc;
  if (N == 0) return GCM_OK;
  HIP_TRY(split_lds_attr(), "ffn split LDS attribute");
  hipStream_t st = (hipStream_t)hip_stream;
  float* part = (float*)workspace;
  with_split_width(C, [&](auto nj, auto nb) {
    constexpr int NJ = decltype(nj)::value, NB = decltype(nb)::value;
    const dim3 grid((unsigned)p.tiles, (unsigned)p.records);
    if (p.split)
      k_ffn_split_forward<NJ, NB, true><<<grid, 256, split_fwd_lds(NJ, NB), st>>>(x, x_stride, ln_w, ln_b, eps, w1, b1, w2, N, C, Hd,
                                                                                  mean, rstd, a, part);
    else
      k_ffn_split_forward<NJ, NB, false><<<grid, 256, split_fwd_lds(NJ, NB), st>>>(x, x_stride, ln_w, ln_b, eps, w1, b1, w2, N, C, Hd,
                                                                                   mean, rstd, a, part);
  });
  HIP_TRY(hipGetLastError(), "ffn split forward launch");
  k_ffn_split_finish<<<blocks_for(N * (C / 4), 256), 256, 0, st>>>(part, (int)p.records, x, x_stride, b2, row_scale, N, C, y, y_stride);
  HIP_TRY(hipGetLastError(), "ffn split forward finish launch");
  return GCM_OK;
}

int gcm_ffn_split_backward(const float* x, int64_t x_stride, const float* mean, const float* rstd, const float* a,
                           const float* dy, int64_t dy_stride, const float* row_scale, const float* ln_w, const float* ln_b,
                           const float* w1, const float* w2, int64_t N, int32_t C, int32_t Hd, float* dx, int64_t dx_stride,
                           float* dln_w, float* dln_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                           size_t workspace_bytes, void* hip_stream) {
  return ffn_backward("gcm_ffn_split_backward", true, x, x_stride, mean, rstd, a, dy, dy_stride, row_scale, ln_w, ln_b, w1, w2, N, C,
                      Hd, dx, dx_stride, dln_w, dln_b, dw1, db1, dw2, db2, workspace, workspace_bytes, hip_stream);
}

int gcm_front_max_channels(void) { return kFrontMaxChannels; }

int gcm_front_forward(const float* x, int64_t x_stride, const float* s, int64_t s_stride, const float* wc, const float* bc,
                      const float* lnc_w, const float* lnc_b, float eps_c, const float* ln1_w, const float* ln1_b,
                      float eps_1, const float* wq, const float* bq, int64_t N, int32_t C, int32_t O, float* feat,
                      int64_t feat_stride, float* qkv, int64_t qkv_stride, float* t, float* mean_c, float* rstd_c,
                      float* mean_1, float* rstd_1, void* hip_stream) {
  const std::string who("gcm_front_forward");
  if (int rc = check_front_shape(who, N, C, O)) return rc;
  if (!std::isfinite(eps_c) || eps_c < 0.0f || !std::isfinite(eps_1) || eps_1 < 0.0f)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": eps_c and eps_1 must be finite and >= 0");
  if (int rc = check_strides(who, {{x_stride, C}, {s_stride, C}, {feat_stride, C}, {qkv_stride, O}})) return rc;
  if (int rc = check_aligned16(who, {x, s, wc, bc, lnc_w, lnc_b, ln1_w, ln1_b, wq, bq, feat, qkv, t})) return rc;
  if (N == 0) return GCM_OK;
  if (!x || !s || !wc || !bc || !lnc_w || !lnc_b || !ln1_w || !ln1_b || !wq || !bq || !feat || !qkv)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, s, wc, bc, lnc_w, lnc_b, ln1_w, ln1_b, wq, bq, feat or qkv");
  const int stats = (mean_c != nullptr) + (rstd_c != nullptr) + (mean_1 != nullptr) + (rstd_1 != nullptr);
  if ((stats != 0 && stats != 4) || (t != nullptr) != (stats == 4))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": t and the four statistics come together, all or none");
  with_nj(C, [&](auto nj) {
    k_front_forward<decltype(nj)::value><<<blocks_for(N, T), 256, 0, (hipStream_t)hip_stream>>>(
        x, x_stride, s, s_stride, wc, bc, lnc_w, lnc_b, eps_c, ln1_w, ln1_b, eps_1, wq, bq, N, C, O, feat, feat_stride, qkv,
        qkv_stride, t, mean_c, rstd_c, mean_1, rstd_1);
  });
  HIP_TRY(hipGetLastError(), "front forward launch");
  return GCM_OK;
}

size_t gcm_front_backward_workspace_bytes(int64_t N, int32_t C, int32_t O) {
  if (check_front_shape("gcm_front_backward_workspace_bytes", N, C, O)) return 0;
  g_err.clear();
  return front_plan(N, C, O).total;
}

int gcm_front_backward(const float* s, int64_t s_stride, const float* feat, int64_t feat_stride, const float* t,
                       const float* mean_c, const float* rstd_c, const float* mean_1, const float* rstd_1,
                       const float* dfeat, int64_t dfeat_stride, const float* dqkv, int64_t dqkv_stride, const float* wc,
                       const float* lnc_w, const float* ln1_w, const float* ln1_b, const float* wq, int64_t N, int32_t C,
                       int32_t O, float* dx, int64_t dx_stride, float* ds, int64_t ds_stride, float* dwc, float* dbc,
                       float* dlnc_w, float* dlnc_b, float* dln1_w, float* dln1_b, float* dwq, float* dbq, void* workspace,
                       size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_front_backward");
  if (int rc = check_front_shape(who, N, C, O)) return rc;
  if (int rc = check_strides(who, {{s_stride, C}, {feat_stride, C}, {dfeat_stride, C}, {dqkv_stride, O},
                                   {dx_stride, C, dx != nullptr}, {ds_stride, C, ds != nullptr}}))
    return rc;
  if (int rc = check_aligned16(who, {s,  feat, t,   dfeat, dqkv,   wc,     lnc_w,  ln1_w,  ln1_b, wq,
                                     dx, ds,   dwc, dbc,   dlnc_w, dlnc_b, dln1_w, dln1_b, dwq,   dbq}))
    return rc;
  const FrontPlan p = front_plan(N, C, O);
  if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, "gcm_front_backward_workspace_bytes")) return rc;
  if (N > 0 && (!s || !feat || !t || !mean_c || !rstd_c || !mean_1 || !rstd_1 || !dfeat || !dqkv || !wc || !lnc_w || !ln1_w ||
                !ln1_b || !wq))
    return fail(GCM_ERR_INVALID_ARGUMENT,
                who + ": null s, feat, t, mean_c, rstd_c, mean_1, rstd_1, dfeat, dqkv, wc, lnc_w, ln1_w, ln1_b or wq");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0) {  // nothing to sum: the parameter gradients are zeros
    const size_t C4 = (size_t)C * 4;
    return clear_outputs(st, {{dwc, C4 * C, "front backward clear dwc"},
                              {dbc, C4, "front backward clear dbc"},
                              {dlnc_w, C4, "front backward clear dlnc_w"},
                              {dlnc_b, C4, "front backward clear dlnc_b"},
                              {dln1_w, C4, "front backward clear dln1_w"},
                              {dln1_b, C4, "front backward clear dln1_b"},
                              {dwq, C4 * O, "front backward clear dwq"},
                              {dbq, (size_t)O * 4, "front backward clear dbq"}});
  }
  char* ws = (char*)workspace;
  float* dt = (float*)(ws + p.dt);
  const bool ln = dln1_w || dln1_b || dlnc_w || dlnc_b, conv = dwc || dbc, proj = dwq || dbq;
  if (dx || ds || ln || conv) {
    float* lnpart = ln ? (float*)(ws + p.lnpart) : nullptr;
    with_nj(C, [&](auto nj) {
      k_front_bwd_rows<decltype(nj)::value><<<(unsigned)p.tiles, 256, 0, st>>>(
          feat, feat_stride, t, mean_c, rstd_c, mean_1, rstd_1, dfeat, dfeat_stride, dqkv, dqkv_stride, wc, lnc_w, ln1_w, wq, N,
          C, O, dx, dx_stride, ds, ds_stride, dt, lnpart);
    });
    HIP_TRY(hipGetLastError(), "front backward rows launch");
    if (ln) {
      fold_ln_partials(lnpart, (float*)(ws + p.lngroup), p.tiles, p.groups, p.gper, 4, C, dln1_w, dln1_b, dlnc_w, dlnc_b, st);
      HIP_TRY(hipGetLastError(), "front backward LayerNorm fold launch");
    }
  }
  if (conv || proj) {
    const int64_t per = slice_rows(N, p.sw);
    float* part = (float*)(ws + p.wpart);
    const dim3 grid(p.wt, (unsigned)p.sw, (conv ? 1u : 0u) + (proj ? 1u : 0u));
    k_front_dw<<<grid, 256, 0, st>>>(s, s_stride, feat, feat_stride, mean_1, rstd_1, ln1_w, ln1_b, dqkv, dqkv_stride, dt, N,
                                     (int)C, (int)O, per, proj ? 0 : 1, part);
    k_ffn_fold_params<<<blocks_for(front_record(C, O), 256), 256, 0, st>>>(part, p.sw, (int64_t)O * C, (int64_t)C * C, O, C, dwq, dwc,
                                                                          dbq, dbc);
    HIP_TRY(hipGetLastError(), "front backward weight gradient launch");
  }
  return GCM_OK;
}

int gcm_mid_max_channels(void) { return kMidMaxChannels; }

int gcm_mid_slot_plan(const int64_t* order, int64_t T_slots, const int64_t* inverse, int64_t N, int32_t* extra,
                      void* hip_stream) {
  const std::string who("gcm_mid_slot_plan");
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": N out of range");
  if (T_slots < 0 || T_slots >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": T out of range");
  if (T_slots < N) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": T below N");
  if (!aligned8(order) || !aligned8(inverse) || (reinterpret_cast<uintptr_t>(extra) & 3u) != 0)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": order and inverse must be 8-byte aligned, extra 4-byte aligned");
  if (N == 0) return GCM_OK;
  if (!order || !inverse || !extra) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null order, inverse or extra");
  hipStream_t st = (hipStream_t)hip_stream;
  k_mid_fill<<<blocks_for(N, 256), 256, 0, st>>>(extra, N);
  k_mid_slot_plan<<<blocks_for(T_slots, 256), 256, 0, st>>>(order, T_slots, inverse, N, extra);
  HIP_TRY(hipGetLastError(), "mid slot plan launch");
  return GCM_OK;
}

int gcm_mid_gather_forward(const float* x, int64_t x_stride, const int64_t* order, int64_t T_slots, int32_t W, float* y,
                           void* hip_stream) {
  const std::string who("gcm_mid_gather_forward");
  if (T_slots < 0 || T_slots >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": T out of range");
  if (int rc = check_mid_width(who, T_slots, W)) return rc;
  if (int rc = check_strides(who, {{x_stride, W}})) return rc;
  if (int rc = check_aligned16(who, {x, y})) return rc;
  if (!aligned8(order)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": order must be 8-byte aligned");
  if (T_slots == 0) return GCM_OK;
  if (!x || !order || !y) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, order or y");
  k_mid_gather_forward<<<blocks_for(T_slots * (W / 4), 256), 256, 0, (hipStream_t)hip_stream>>>(x, x_stride, order, T_slots,
                                                                                               W / 4, y);
  HIP_TRY(hipGetLastError(), "mid gather forward launch");
  return GCM_OK;
}

int gcm_mid_gather_backward(const float* dy, int64_t dy_stride, const int64_t* inverse, const int32_t* extra, int64_t N,
                            int32_t W, float* dx, void* hip_stream) {
  const std::string who("gcm_mid_gather_backward");
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": N out of range");
  if (int rc = check_mid_width(who, N, W)) return rc;
  if (int rc = check_strides(who, {{dy_stride, W}})) return rc;
  if (int rc = check_aligned16(who, {dy, dx})) return rc;
  if (!aligned8(inverse) || (reinterpret_cast<uintptr_t>(extra) & 3u) != 0)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": inverse must be 8-byte aligned, extra 4-byte aligned");
  if (N == 0) return GCM_OK;
  if (!dy || !inverse || !extra || !dx) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null dy, inverse, extra or dx");
  k_mid_gather_backward<<<blocks_for(N * (W / 4), 256), 256, 0, (hipStream_t)hip_stream>>>(dy, dy_stride, inverse, extra, N,
                                                                                          W / 4, dx);
  HIP_TRY(hipGetLastError(), "mid gather backward launch");
  return GCM_OK;
}

int gcm_mid_forward(const float* a, int64_t a_stride, const int64_t* inverse, const float* x, int64_t x_stride,
                    const float* wp, const float* bp, const float* row_scale, int64_t N, int32_t C, float* y,
                    int64_t y_stride, void* hip_stream) {
  const std::string who("gcm_mid_forward");
  if (int rc = check_mid_shape(who, N, C)) return rc;
  if (int rc = check_strides(who, {{a_stride, C}, {x_stride, C}, {y_stride, C}})) return rc;
  if (int rc = check_aligned16(who, {a, x, wp, bp, y})) return rc;
  if (!aligned8(inverse)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": inverse must be 8-byte aligned");
  if (N == 0) return GCM_OK;
  if (!a || !inverse || !x || !wp || !bp || !y) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null a, inverse, x, wp, bp or y");
  with_nj(C, [&](auto nj) {
    k_mid_forward<decltype(nj)::value><<<blocks_for(N, T), 256, 0, (hipStream_t)hip_stream>>>(a, a_stride, inverse, x, x_stride, wp,
                                                                                             bp, row_scale, N, C, y, y_stride);
  });
  HIP_TRY(hipGetLastError(), "mid forward launch");
  return GCM_OK;
}

size_t gcm_mid_backward_workspace_bytes(int64_t N, int32_t C) {
  if (check_mid_shape("gcm_mid_backward_workspace_bytes", N, C)) return 0;
  g_err.clear();
  return mid_plan(N, C).total;
}

int gcm_mid_backward(const float* a, int64_t a_stride, const int64_t* inverse, const int32_t* extra, const float* dy,
                     int64_t dy_stride, const float* wp, const float* row_scale, int64_t N, int64_t T_slots, int32_t C,
                     float* da, float* dwp, float* dbp, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_mid_backward");
  if (int rc = check_mid_shape(who, N, C)) return rc;
  if (T_slots < 0 || T_slots >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": T out of range");
  if (T_slots < N) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": T below N");
  if (int rc = check_strides(who, {{a_stride, C}, {dy_stride, C}})) return rc;
  if (int rc = check_aligned16(who, {a, dy, wp, da, dwp, dbp})) return rc;
  if (!aligned8(inverse) || (reinterpret_cast<uintptr_t>(extra) & 3u) != 0)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": inverse must be 8-byte aligned, extra 4-byte aligned");
  const MidPlan p = mid_plan(N, C);
  if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, "gcm_mid_backward_workspace_bytes")) return rc;
  if (N > 0 && (!a || !inverse || !extra || !dy || !wp))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null a, inverse, extra, dy or wp");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0)  // no row owns a slot: every gradient is zeros
    return clear_outputs(st, {{T_slots ? da : nullptr, (size_t)T_slots * C * 4, "mid backward clear da"},
                              {dwp, (size_t)C * C * 4, "mid backward clear dwp"},
                              {dbp, (size_t)C * 4, "mid backward clear dbp"}});
  if (da) {
    with_nj(C, [&](auto nj) {
      k_mid_bwd_rows<decltype(nj)::value><<<(unsigned)p.tiles, 256, 0, st>>>(dy, dy_stride, inverse, extra, wp, row_scale, N,
                                                                            T_slots, C, da);
    });
    HIP_TRY(hipGetLastError(), "mid backward rows launch");
  }
  if (dwp || dbp) {
    const int64_t per = slice_rows(N, p.sw);
    float* part = (float*)workspace;
    k_mid_dw<<<dim3(p.wt, (unsigned)p.sw), 256, 0, st>>>(a, a_stride, inverse, dy, dy_stride, row_scale, N, T_slots, (int)C, per,
                                                         part);
    k_ffn_fold_params<<<blocks_for(mid_record(C), 256), 256, 0, st>>>(part, p.sw, (int64_t)C * C, C, 0, 0, dwp, dbp, nullptr,
                                                                     nullptr);
    HIP_TRY(hipGetLastError(), "mid backward weight gradient launch");
  }
  return GCM_OK;
}

int gcm_seam_max_channels(void) { return kSeamMaxChannels; }

int gcm_seam_forward_eval(const float* x, int64_t x_stride, const float* w, const float* b, const float* running_mean,
                          const float* running_var, float eps, const float* bn_w, const float* bn_b, int act, int64_t N,
                          int32_t I, int32_t O, float* y, int64_t y_stride, float* z, float* rstd, void* hip_stream) {
  const std::string who("gcm_seam_forward_eval");
  if (int rc = check_seam_shape(who, N, I, O, w != nullptr)) return rc;
  if (!std::isfinite(eps) || eps < 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": eps must be finite and >= 0");
  if (int rc = check_strides(who, {{x_stride, I}, {y_stride, O}})) return rc;
  if (int rc = check_aligned16(who, {x, w, b, running_mean, running_var, bn_w, bn_b, y, z, rstd})) return rc;
  if (!w && (b || z)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": b and z need w (without it z is x itself)");
  if (N == 0) return GCM_OK;
  if (!x || !running_mean || !running_var || !bn_w || !bn_b || !y)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, running_mean, running_var, bn_w, bn_b or y");
  hipStream_t st = (hipStream_t)hip_stream;
  if (w) {
    with_nj(O, [&](auto nj) {  // the column block: the narrowest instantiation that holds O, else 128 columns a block
      constexpr int NJ = decltype(nj)::value;
      k_seam_forward<NJ, true><<<dim3(blocks_for(N, T), blocks_for(O, 32 * NJ)), 256, 0, st>>>(
          x, x_stride, w, b, running_mean, running_var, eps, bn_w, bn_b, act, N, I, O, z, y, y_stride, rstd, nullptr);
    });
  } else {
    k_seam_apply<true><<<blocks_for(N * (O / 4), 256), 256, 0, st>>>(x, x_stride, running_mean, running_var, eps, bn_w, bn_b, act,
                                                                     N, O / 4, y, y_stride, rstd);
  }
  HIP_TRY(hipGetLastError(), "seam forward launch");
  return GCM_OK;
}

size_t gcm_seam_forward_workspace_bytes(int64_t N, int32_t O) {
  if (check_seam_shape("gcm_seam_forward_workspace_bytes", N, 4, O, true)) return 0;
  g_err.clear();
  return seam_forward_bytes(N, O);
}

int gcm_seam_forward_train(const float* x, int64_t x_stride, const float* w, const float* b, float eps, float momentum,
                           const float* bn_w, const float* bn_b, int act, int64_t N, int32_t I, int32_t O, float* z, float* y,
                           int64_t y_stride, float* mean, float* rstd, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_seam_forward_train");
  if (int rc = check_seam_shape(who, N, I, O, w != nullptr)) return rc;
  if (!std::isfinite(eps) || eps < 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": eps must be finite and >= 0");
  if (!std::isfinite(momentum) || momentum < 0.0f || momentum > 1.0f)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": momentum must be in 0..1");
  if (int rc = check_strides(who, {{x_stride, I}, {y_stride, O}})) return rc;
  if (int rc = check_aligned16(who, {x, w, b, bn_w, bn_b, z, y, mean, rstd, running_mean, running_var})) return rc;
  if (!aligned8(num_batches_tracked)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": num_batches_tracked must be 8-byte aligned");
  if (!w && (b || z)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": b and z need w (without it z is x itself)");
  const int buffers = (running_mean != nullptr) + (running_var != nullptr) + (num_batches_tracked != nullptr);
  if (buffers != 0 && buffers != 3)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": running_mean, running_var and num_batches_tracked come together, all or none");
  if (N == 0) return GCM_OK;
  if (N < 2) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": batch statistics need N >= 2");
  const size_t need = seam_forward_bytes(N, O);
  if (int rc = check_workspace(who, workspace, workspace_bytes, need, "gcm_seam_forward_workspace_bytes")) return rc;
  if (!x || !bn_w || !bn_b || !y || !mean || !rstd || (w && !z))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, bn_w, bn_b, y, mean, rstd or (with w) z");
  hipStream_t st = (hipStream_t)hip_stream;
  const SeamPlan p = seam_plan(N, I, O);
  float* part = (float*)workspace;
  if (w) {
    with_nj(O, [&](auto nj) {
      constexpr int NJ = decltype(nj)::value;
      k_seam_forward<NJ, false><<<dim3((unsigned)p.tiles, blocks_for(O, 32 * NJ)), 256, 0, st>>>(
          x, x_stride, w, b, nullptr, nullptr, eps, bn_w, bn_b, act, N, I, O, z, nullptr, 0, nullptr, part);
    });
  } else {
    k_seam_tile_stats<<<dim3((unsigned)p.tiles, blocks_for(O, kSeamChunk)), 256, 0, st>>>(x, x_stride, N, (int)O, part);
  }
  HIP_TRY(hipGetLastError(), "seam product launch");
  k_seam_stats<<<blocks_for(O, 4), 256, 0, st>>>(part, p.tiles, N, (int)O, p.G, p.gper, eps, momentum, mean, rstd, running_mean,
                                                running_var, num_batches_tracked);
  HIP_TRY(hipGetLastError(), "seam statistics launch");
  k_seam_apply<false><<<blocks_for(N * (O / 4), 256), 256, 0, st>>>(w ? z : x, w ? (int64_t)O : x_stride, mean, rstd, eps, bn_w,
                                                                    bn_b, act, N, O / 4, y, y_stride, (float*)nullptr);
  HIP_TRY(hipGetLastError(), "seam apply launch");
  return GCM_OK;
}

size_t gcm_seam_backward_workspace_bytes(int64_t N, int32_t I, int32_t O) {
  if (check_seam_shape("gcm_seam_backward_workspace_bytes", N, I, O, true)) return 0;
  g_err.clear();
  return seam_plan(N, I, O).total;
}

int gcm_seam_backward(const float* x, int64_t x_stride, const float* z, int64_t z_stride, const float* mean,
                      const float* rstd, const float* dy, int64_t dy_stride, const float* w, const float* bn_w,
                      const float* bn_b, int act, int batch_stats, int64_t N, int32_t I, int32_t O, float* dx,
                      int64_t dx_stride, float* dw, float* db, float* dbn_w, float* dbn_b, void* workspace,
                      size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_seam_backward");
  if (int rc = check_seam_shape(who, N, I, O, w != nullptr)) return rc;
  if (int rc = check_strides(who, {{x_stride, I}, {z_stride, O}, {dy_stride, O}, {dx_stride, I, dx != nullptr}})) return rc;
  if (int rc = check_aligned16(who, {x, z, mean, rstd, dy, w, bn_w, bn_b, dx, dw, db, dbn_w, dbn_b})) return rc;
  if (!w && (dw || db)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": dw and db need w");
  if (batch_stats && N == 1) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": batch statistics need N >= 2");
  const SeamPlan p = seam_plan(N, I, O);
  if (int rc = check_workspace(who, workspace, workspace_bytes, p.total, "gcm_seam_backward_workspace_bytes")) return rc;
  if (N > 0 && (!z || !mean || !rstd || !dy || !bn_w || !bn_b || (w && !x)))
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null z, mean, rstd, dy, bn_w, bn_b or (with w) x");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0)  // nothing to sum: the parameter gradients are zeros
    return clear_outputs(st, {{dw, (size_t)O * I * 4, "seam backward clear dw"},
                              {db, (size_t)O * 4, "seam backward clear db"},
                              {dbn_w, (size_t)O * 4, "seam backward clear dbn_w"},
                              {dbn_b, (size_t)O * 4, "seam backward clear dbn_b"}});
  char* ws = (char*)workspace;
  float* keep = (float*)(ws + p.keep);
  const bool rows = dx || dw || db;  // what reads dz
  if (dbn_w || dbn_b || (batch_stats && rows)) {
    float* part = (float*)(ws + p.part);
    k_seam_bwd_part<<<dim3((unsigned)p.tiles, blocks_for(O, T)), 256, 0, st>>>(dy, dy_stride, z, z_stride, mean, rstd, bn_w, bn_b,
                                                                              act, N, (int)O, part);
    k_seam_bwd_fold<<<blocks_for(O, 4), 256, 0, st>>>(part, p.tiles, (int)O, p.G, p.gper, dbn_w, dbn_b, keep);
    HIP_TRY(hipGetLastError(), "seam backward BatchNorm sums launch");
  }
  SeamDz d;
  d.dy = dy, d.z = z, d.mean = mean, d.rstd = rstd, d.gam = bn_w, d.bet = bn_b;
  d.kh = batch_stats ? keep : nullptr, d.kg = batch_stats ? keep + O : nullptr;
  d.dys = dy_stride, d.zs = z_stride, d.inv_n = 1.0f / (float)N, d.act = act;
  if (dx) {
    if (w)
      with_nj(I, [&](auto nj) {
        constexpr int NJ = decltype(nj)::value;
        k_seam_dx<NJ><<<dim3((unsigned)p.tiles, blocks_for(I, 32 * NJ)), 256, 0, st>>>(d, w, N, I, O, dx, dx_stride);
      });
    else k_seam_dz<<<blocks_for(N * (O / 4), 256), 256, 0, st>>>(d, N, O / 4, dx, dx_stride);
    HIP_TRY(hipGetLastError(), "seam backward dx launch");
  }
  if (dw || db) {
    const int64_t per = slice_rows(N, p.sw);
    float* part = (float*)(ws + p.wpart);
    k_seam_dw<<<dim3(p.wt, (unsigned)p.sw), 256, 0, st>>>(d, x, x_stride, N, (int)I, (int)O, per, part);
    k_ffn_fold_params<<<blocks_for(seam_record(I, O), 256), 256, 0, st>>>(part, p.sw, (int64_t)O * I, O, 0, 0, dw, db, nullptr,
                                                                         nullptr);
    HIP_TRY(hipGetLastError(), "seam backward weight gradient launch");
  }
  return GCM_OK;
}

int gcm_head_chain_max_hidden(void) { return kChainMaxHidden; }
int gcm_head_chain_max_in(void) { return kChainMaxIn; }

int gcm_head_chain(const float* x, int64_t x_stride, const float* onehots, int64_t onehots_stride, const float* w1,
                   int64_t w1_stride, const float* b1, const float* w_ma, const float* w2, int64_t w2_stride,
                   const float* alpha, const float* beta, const float* bias2, const int32_t* group, const float* w_out,
                   const float* b_out, int64_t N, int32_t I, int32_t K, int32_t H, int32_t G, int32_t C, int kind,
                   float factor, float slope, float* out, void* hip_stream) {
  const std::string who("gcm_head_chain");
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": N out of range");
  if (I <= 0 || I % 4 != 0 || I > kChainMaxIn)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": I must be a positive multiple of 4, at most gcm_head_chain_max_in()");
  if (H <= 0 || H % 4 != 0 || H > kChainMaxHidden)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": H must be a positive multiple of 4, at most gcm_head_chain_max_hidden()");
  if (K < 1 || K > kChainMaxClasses) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": K must be in 1..32");
  if (G < 1 || G > kMaxGroups) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": G must be in 1..2^20");
  if (C != 1 && C != 3) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": C must be 1 or 3");
  if (kind != GCM_XYZ && kind != GCM_RGB && kind != GCM_SCALE && kind != GCM_OPACITY)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": unknown kind");
  if (!std::isfinite(factor)) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": factor is not finite");
  if (!std::isfinite(slope) || slope <= 0.0f) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": slope must be finite and > 0");
  if (int rc = check_strides(who, {{x_stride, I}, {w1_stride, I}, {w2_stride, H}})) return rc;
  if (onehots_stride < K) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": onehots_stride below K");
  if (int rc = check_aligned16(who, {x, w1, b1, w_ma, w2, alpha, beta, bias2, w_out, b_out, out})) return rc;
  if ((reinterpret_cast<uintptr_t>(onehots) & 3u) != 0 || (reinterpret_cast<uintptr_t>(group) & 3u) != 0)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": onehots and group must be 4-byte aligned");
  if (N == 0) return GCM_OK;
  if (!x || !onehots || !w1 || !b1 || !w_ma || !w2 || !w_out || !out)
    return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null x, onehots, w1, b1, w_ma, w2, w_out or out");
  HIP_TRY(chain_lds_attr(), "head_chain LDS attribute");
  ChainArgs a;
  a.x = x, a.onehots = onehots, a.w1 = w1, a.b1 = b1, a.wma = w_ma, a.w2 = w2, a.alpha = alpha, a.beta = beta, a.bias2 = bias2;
  a.wout = w_out, a.bout = b_out, a.group = group, a.out = out;
  a.xs = x_stride, a.os = onehots_stride, a.w1s = w1_stride, a.w2s = w2_stride, a.N = N;
  a.I = I, a.K = K, a.H = H, a.G = G, a.kind = kind, a.factor = factor, a.slope = slope;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t lds = chain_lds_bytes(H);
  if (C == 1) k_head_chain<1><<<blocks_for(N, T), kChainThreads, lds, st>>>(a);
  else k_head_chain<3><<<blocks_for(N, T), kChainThreads, lds, st>>>(a);
  HIP_TRY(hipGetLastError(), "head_chain launch");
  return GCM_OK;
}

}  // extern "C"

int gcm_head_train_max_in(void) { return kHeadTrainMaxIn; }
int gcm_head_train_pre_floats(void) { return kHeadPreFloats; }

namespace {

int check_head_train_shape(const std::string& w, int64_t N, int32_t I) {
  if (N < 0 || N >= kMaxRows) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": N out of range");
  if (I <= 0 || I % 4 != 0 || I > kHeadTrainMaxIn)
    return fail(GCM_ERR_INVALID_ARGUMENT, w + ": I must be a positive multiple of 4, at most gcm_head_train_max_in()");
  return 0;
}

// what the forward and the backward ask of every key; packed: the [N][14] form, so no key may carry out / dout
int check_head_keys(const std::string& w, const gcm_head_key* keys, int32_t n_keys, int64_t N, int32_t I, bool backward,
                    bool packed, HeadKeys& hk) {
  if (n_keys < 1 || n_keys > 4) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": n_keys must be in 1..4");
  if (!keys) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": null keys");
  int seen = 0;
  for (int k = 0; k < n_keys; k++) {
    const gcm_head_key& key = keys[k];
    if (key.kind != GCM_XYZ && key.kind != GCM_RGB && key.kind != GCM_SCALE && key.kind != GCM_OPACITY)
      return fail(GCM_ERR_INVALID_ARGUMENT, w + ": unknown kind");
    if (seen >> key.kind & 1) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": a kind is given twice");
    seen |= 1 << key.kind;
    if (!std::isfinite(key.factor)) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": factor is not finite");
    const int C = head_channels(key.kind);
    if (int rc = check_strides(w, {{key.h_stride, I}, {key.dh_stride, I, backward && key.dh != nullptr}})) return rc;
    const void* form = backward ? (const void*)key.dout : (const void*)key.out;
    if (form ? packed : (!packed && N > 0))  // without rows torch's empty tensors are null pointers: no form to tell
      return fail(GCM_ERR_INVALID_ARGUMENT,
                  w + (backward ? ": give every key's dout or dpoints14, not both and not neither"
                                : ": give every key's out or points14, not both and not neither"));
    if (form && (backward ? key.dout_stride : key.out_stride) < C)
      return fail(GCM_ERR_INVALID_ARGUMENT, w + ": the row stride of out / dout must be at least C");
    if (int rc = check_aligned16(w, {key.h, key.w})) return rc;
    if (backward)
      if (int rc = check_aligned16(w, {key.dh, key.dw})) return rc;
    if (N > 0 && (!key.h || !key.w)) return fail(GCM_ERR_INVALID_ARGUMENT, w + ": null h or w");
    hk.k[k] = key;
  }
  hk.n = n_keys;
  return 0;
}

}  // namespace

int gcm_head_train_plan(int64_t N, int32_t I, int64_t* plan) {
  const std::string who("gcm_head_train_plan");
  if (int rc = check_head_train_shape(who, N, I)) return rc;
  if (!plan) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null plan");
  const HeadTrainPlan p = head_train_plan(N, I);
  const int64_t v[8] = {p.tiles, p.tpb, p.records, p.groups, p.per, p.levels, p.rec_floats, p.key_floats};
  std::copy(v, v + 8, plan);
  return GCM_OK;
}

size_t gcm_head_train_workspace_bytes(int64_t N, int32_t I, int32_t n_keys) {
  const std::string who("gcm_head_train_workspace_bytes");
  if (check_head_train_shape(who, N, I)) return 0;
  if (n_keys < 1 || n_keys > 4) {
    fail(GCM_ERR_INVALID_ARGUMENT, who + ": n_keys must be in 1..4");
    return 0;
  }
  g_err.clear();
  return round256((size_t)head_train_plan(N, I).key_floats * n_keys * 4);
}

int gcm_head_train_forward(const gcm_head_key* keys, int32_t n_keys, const int32_t* group, int64_t N, int32_t I, float* pre,
                           const float* xyz, int64_t xyz_stride, const float* scales, int64_t scales_stride,
                           float* points14, void* hip_stream) {
  const std::string who("gcm_head_train_forward");
  if (int rc = check_head_train_shape(who, N, I)) return rc;
  HeadKeys hk;
  if (int rc = check_head_keys(who, keys, n_keys, N, I, false, points14 != nullptr, hk)) return rc;
  if (points14) {
    bool rgb = false;
    for (int k = 0; k < n_keys; k++) rgb = rgb || keys[k].kind == GCM_RGB;
    if (!rgb || !xyz || !scales) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": points14 needs the rgb key, xyz and scales");
    if (xyz_stride < 3 || scales_stride < 3)
      return fail(GCM_ERR_INVALID_ARGUMENT, who + ": the row strides of xyz and scales must be at least 3");
  }
  if (N == 0) return GCM_OK;
  k_head_train_fwd<<<blocks_for(N, 16), 256, 0, (hipStream_t)hip_stream>>>(hk, group, N, I, pre, xyz, xyz_stride, scales,
                                                                           scales_stride, points14);
  HIP_TRY(hipGetLastError(), "head train forward launch");
  return GCM_OK;
}

int gcm_head_train_backward(const gcm_head_key* keys, int32_t n_keys, const int32_t* group, int64_t N, int32_t I,
                            const float* pre, const float* scales, int64_t scales_stride, const float* dpoints14,
                            int64_t dpoints_stride, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const std::string who("gcm_head_train_backward");
  if (int rc = check_head_train_shape(who, N, I)) return rc;
  HeadKeys hk;
  if (int rc = check_head_keys(who, keys, n_keys, N, I, true, dpoints14 != nullptr, hk)) return rc;
  if (dpoints14) {
    if (dpoints_stride < 14) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": dpoints_stride must be at least 14");
    for (int k = 0; k < n_keys; k++)
      if (keys[k].kind == GCM_SCALE && (!scales || scales_stride < 3))
        return fail(GCM_ERR_INVALID_ARGUMENT, who + ": dpoints14 with the scale key needs scales, row stride at least 3");
  }
  const HeadTrainPlan p = head_train_plan(N, I);
  const size_t need = round256((size_t)p.key_floats * n_keys * 4);
  if (int rc = check_workspace(who, workspace, workspace_bytes, need, "gcm_head_train_workspace_bytes")) return rc;
  if (N > 0 && !pre) return fail(GCM_ERR_INVALID_ARGUMENT, who + ": null pre");
  hipStream_t st = (hipStream_t)hip_stream;
  if (N == 0) {
    for (int k = 0; k < n_keys; k++) {
      const size_t C = (size_t)head_channels(keys[k].kind);
      if (int rc = clear_outputs(st, {{keys[k].dw, C * I * 4, "head train clear dw"}, {keys[k].db, C * 4, "head train clear db"}}))
        return rc;
    }
    return GCM_OK;
  }
  float* records = (float*)workspace;
  k_head_train_rows<<<dim3((unsigned)p.records, (unsigned)n_keys), 256, 0, st>>>(
      hk, group, N, I, pre, scales, scales_stride, dpoints14, dpoints_stride, p.tiles, (int)p.tpb, p.rec_floats, p.key_floats,
      records);
  HIP_TRY(hipGetLastError(), "head train rows launch");
  k_head_train_fold<<<dim3(blocks_for(3 * (int64_t)I + 3, 16), (unsigned)n_keys), 256, 0, st>>>(
      hk, I, p.records, p.per, (int)p.groups, p.rec_floats, p.key_floats, records);
  HIP_TRY(hipGetLastError(), "head train fold launch");
  return GCM_OK;
}
