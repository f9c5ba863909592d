// gca_attention.hip -- MI355X (gfx950) kernels + C ABI (include/gca.h) of the point backbone's attention:
// variable-length, packed-QKV, non-causal softmax attention in binary16 (flash_attn_varlen_qkvpacked_func).
// DESIGN.md section 16.
//
// Every product is a v_mfma_f32_16x16x16_f16 (fp32 accumulation).  Its operand maps, lane l, c = l & 15, g = l >> 4:
//   A[row c][k 4g + j], B[k 4g + j][col c] (j = 0..3, one 8-byte fragment), C/D[row 4g + r][col c] (r = 0..3).
// A C/D tile is therefore already the B fragment of a following product that sums over the tile's ROW index, and
// the orientation of every first product is chosen for that:
//   forward   S^T = K Q^T  (key on the register, query on the lane)   ->  O^T += V^T P^T
//   dQ pass   S^T = K Q^T, dP^T = V dO^T, dS^T                        ->  dQ^T += K^T dS^T
//   dK/dV     S = Q K^T, dP = dO V^T (query on the register, key on the lane) -> dV^T += dO^T P, dK^T += Q^T dS
// so neither P nor dS ever passes through LDS, and every result tile has four consecutive channels of one row
// on a lane (one 8-byte store).  The operand that stays (Q and dO of a query tile; K and V of a key tile) lives
// in registers; the streamed one is staged in LDS in blocks, row-major for the fragments read by rows and
// transposed (row pitch = 8 mod 64 words, conflict-free 8-byte reads) for those read by columns.
//
// A workgroup is 4 waves = 64 rows of one (segment, head): 16 per wave.  The next staged block's global loads are
// issued before the current block is computed on.  The forward keeps a running fp32 maximum
// and per-lane partial row sums over blocks of 64 keys (two lane exchanges per block for the maximum, two per row
// for the sum at the end).  The backward recomputes P from the saved log-sum-exp; one pass owns key tiles (dK, dV),
// one owns query tiles (dQ): every sum has a fixed order, there are no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/gca.h"
#define GC_ERR_HIP GCA_ERR_HIP
#include "gc_host.h"

namespace {

typedef _Float16 half_t;
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef unsigned u2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;  // 4 waves
constexpr int kRowsPerGroup = 64;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

__device__ __forceinline__ f4 mfma(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ h4 ld4(const half_t* p) { return *reinterpret_cast<const h4*>(p); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }  // v_exp_f32
__device__ __forceinline__ h4 to_half(f4 v) { return __builtin_convertvector(v, h4); }

template <int ND, int NB>
struct Tile {
  static constexpr int D = 16 * ND;
  static constexpr int KS = ND == 1 ? 16 : D + 4;  // row-major pitch (halves): 8-byte fragments spread over the banks
  static constexpr int VS = NB + 16;               // transposed pitch: 72 / 40 words = 8 mod 64 / 40 mod 64
};

// Segment s of the clamped cu_seqlens: first row and length (cut to max_seqlen).
__device__ __forceinline__ void segment(const int32_t* cu, int64_t seg, int64_t total, int max_seqlen, int64_t& beg, int& len) {
  int64_t b = cu[seg], e = cu[seg + 1];
  b = b < 0 ? 0 : (b > total ? total : b);
  e = e < 0 ? 0 : (e > total ? total : e);
  int64_t n = e - b;
  n = n < 0 ? 0 : (n > max_seqlen ? max_seqlen : n);
  beg = b;
  len = (int)n;
}

// Staging of rows r0 .. r0 + NB - 1 of one (slot, head) -- `base` is row 0 of the segment -- in two halves, so that
// the global loads of the next block are in flight while the current one is computed on: stage_load fills the
// thread's registers (rows at or beyond `len` are zeros), stage_store writes them to LDS, row-major Xs [NB][KS]
// and / or transposed Xt [D][VS].
template <int ND, int NB>
struct Staged {
  static constexpr int CPR = 2 * ND;                                     // 16-byte pieces per row
  static constexpr int N = (NB * CPR + kThreads - 1) / kThreads;         // pieces per thread
  u4 v[N];
};

template <int ND, int NB>
__device__ __forceinline__ void stage_load(Staged<ND, NB>& st, const half_t* base, int64_t rs, int r0, int len) {
  typedef Staged<ND, NB> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) {
    const int idx = threadIdx.x + i * kThreads;
    const int row = idx / S::CPR, cc = idx % S::CPR;
    st.v[i] = u4{0u, 0u, 0u, 0u};
    if (idx < NB * S::CPR && r0 + row < len) st.v[i] = *reinterpret_cast<const u4*>(base + (int64_t)(r0 + row) * rs + cc * 8);
  }
}

template <int ND, int NB, bool ROW, bool TR>
__device__ __forceinline__ void stage_store(const Staged<ND, NB>& st, half_t* Xs, half_t* Xt) {
  typedef Tile<ND, NB> T;
  typedef Staged<ND, NB> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) {
    const int idx = threadIdx.x + i * kThreads;
    if (idx >= NB * S::CPR) break;
    const int row = idx / S::CPR, cc = idx % S::CPR;
    const u4 v = st.v[i];
    if (ROW) {
      u2 lo = {v.x, v.y}, hi = {v.z, v.w};
      *reinterpret_cast<u2*>(Xs + row * T::KS + cc * 8) = lo;
      *reinterpret_cast<u2*>(Xs + row * T::KS + cc * 8 + 4) = hi;
    }
    if (TR) {
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        reinterpret_cast<unsigned short*>(Xt)[(cc * 8 + 2 * j) * T::VS + row] = (unsigned short)(w[j] & 0xffffu);
        reinterpret_cast<unsigned short*>(Xt)[(cc * 8 + 2 * j + 1) * T::VS + row] = (unsigned short)(w[j] >> 16);
      }
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------
// 64 keys (LDS rows c0 .. c0 + 63) against the wave's 16 queries: S^T tiles, running maximum `m` (in units of
// log2, shared by the four lanes of a query), per-lane partial row sums `lv`, O^T += V^T P^T.  MASK: only the
// first `valid` keys are inside the segment.
template <int ND, int NB, bool MASK>
__device__ __forceinline__ void forward_step(const half_t* Ks, const half_t* Vt, const h4 (&qf)[ND], f4 (&o)[ND], float& m,
                                             f4& lv, float sl2, int c0, int c, int g, int valid) {
  typedef Tile<ND, NB> T;
  f4 s[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    s[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) s[t] = mfma(ld4(Ks + (c0 + t * 16 + c) * T::KS + kd * 16 + 4 * g), qf[kd], s[t]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    s[t] = s[t] * sl2;
    if (MASK) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t * 16 + 4 * g + r >= valid) s[t][r] = -INFINITY;
    }
  }
  float mx = fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3]));
#pragma unroll
  for (int t = 1; t < 4; ++t) mx = fmaxf(fmaxf(fmaxf(mx, s[t][0]), fmaxf(s[t][1], s[t][2])), s[t][3]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float mn = fmaxf(m, mx);  // finite: the first key of the step is inside the segment
  const float alpha = ex2(m - mn);
  m = mn;
  lv = lv * alpha;
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) o[kd] = o[kd] * alpha;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f4 e = s[t] - mn;
    f4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = ex2(e[r]);
    lv = lv + p;
    const h4 ph = to_half(p);
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) o[kd] = mfma(ld4(Vt + (kd * 16 + c) * T::VS + c0 + t * 16 + 4 * g), ph, o[kd]);
  }
}

template <int ND>
__global__ __launch_bounds__(kThreads) void k_forward(const half_t* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                      const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                      int qblocks, float sl2, half_t* __restrict__ out,
                                                      float* __restrict__ lse, int heads) {
  constexpr int NB = 128;
  typedef Tile<ND, NB> T;
  constexpr int D = T::D;
  __shared__ __align__(16) half_t Ks[NB * T::KS];
  __shared__ __align__(16) half_t Vt[D * T::VS];
  const int64_t seg = blockIdx.x / qblocks;
  const int q0 = (int)(blockIdx.x % qblocks) * kRowsPerGroup;
  const int h = blockIdx.z;
  int64_t beg;
  int len;
  segment(cu, seg, total, max_seqlen, beg, len);
  if (q0 >= len) return;  // uniform over the workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qrow = q0 + wave * 16 + c;
  const bool qvalid = qrow < len;
  const half_t* seg_base = qkv + beg * rs + (int64_t)h * hs;
  h4 qf[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    qf[kd] = h4{0, 0, 0, 0};
    if (qvalid) qf[kd] = ld4(seg_base + (int64_t)qrow * rs + kd * 16 + 4 * g);
  }
  f4 o[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) o[kd] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY;
  f4 lv = {0.f, 0.f, 0.f, 0.f};

  Staged<ND, NB> kst, vst;
  stage_load(kst, seg_base + ss, rs, 0, len);
  stage_load(vst, seg_base + 2 * ss, rs, 0, len);
  for (int kb = 0; kb < len; kb += NB) {
    __syncthreads();
    stage_store<ND, NB, true, false>(kst, Ks, nullptr);
    stage_store<ND, NB, false, true>(vst, nullptr, Vt);
    __syncthreads();
    if (kb + NB < len) {
      stage_load(kst, seg_base + ss, rs, kb + NB, len);
      stage_load(vst, seg_base + 2 * ss, rs, kb + NB, len);
    }
    const int nk = len - kb < NB ? len - kb : NB;
    // keys beyond the segment exist only in its last block of 64, which takes the masked copy of the step
    for (int c0 = 0; c0 < nk; c0 += 64) {
      if (c0 + 64 <= nk)
        forward_step<ND, NB, false>(Ks, Vt, qf, o, m, lv, sl2, c0, c, g, 64);
      else
        forward_step<ND, NB, true>(Ks, Vt, qf, o, m, lv, sl2, c0, c, g, nk - c0);
    }
  }
  float l = (lv[0] + lv[1]) + (lv[2] + lv[3]);
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qvalid) {
    half_t* orow = out + ((beg + qrow) * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) {
      f4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = o[kd][r] / l;
      *reinterpret_cast<h4*>(orow + kd * 16 + 4 * g) = to_half(v);
    }
    if (g == 0) lse[(int64_t)h * total + beg + qrow] = (m + log2f(l)) * kLn2;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
// delta[h][row] = sum_c dout[row][h][c] * out[row][h][c], fp32, channels in order.
template <int ND>
__global__ __launch_bounds__(kThreads) void k_delta(const half_t* __restrict__ out, const half_t* __restrict__ dout,
                                                    int64_t drs, int64_t dhs, int64_t total, int heads,
                                                    float* __restrict__ delta) {
  constexpr int D = 16 * ND;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total * heads) return;
  const int64_t row = idx / heads;
  const int h = (int)(idx % heads);
  const half_t* o = out + idx * D;
  const half_t* d = dout + row * drs + (int64_t)h * dhs;
  float acc = 0.f;
#pragma unroll
  for (int cc = 0; cc < D / 8; ++cc) {
    const u4 a = *reinterpret_cast<const u4*>(o + cc * 8), b = *reinterpret_cast<const u4*>(d + cc * 8);
    const half_t* ah = reinterpret_cast<const half_t*>(&a);
    const half_t* bh = reinterpret_cast<const half_t*>(&b);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += (float)ah[i] * (float)bh[i];
  }
  delta[(int64_t)h * total + row] = acc;
}

// dK, dV: a wave owns 16 keys (K, V fragments in registers) and streams the segment's queries through LDS.
template <int ND>
__global__ __launch_bounds__(kThreads) void k_backward_kv(const half_t* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                          const half_t* __restrict__ dout, int64_t drs, int64_t dhs,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                          int kblocks, float sl2, float scale, half_t* __restrict__ dqkv,
                                                          int heads) {
  constexpr int NB = ND <= 2 ? 128 : 64;  // queries per staged block (LDS: 19 / 37 / 38 KB at d = 16 / 32 / 64)
  typedef Tile<ND, NB> T;
  constexpr int D = T::D;
  __shared__ __align__(16) half_t Qs[NB * T::KS];
  __shared__ __align__(16) half_t Qt[D * T::VS];
  __shared__ __align__(16) half_t Os[NB * T::KS];
  __shared__ __align__(16) half_t Ot[D * T::VS];
  __shared__ __align__(16) float Ls[NB];
  __shared__ __align__(16) float Ds[NB];
  const int64_t seg = blockIdx.x / kblocks;
  const int k0 = (int)(blockIdx.x % kblocks) * kRowsPerGroup;
  const int h = blockIdx.z;
  int64_t beg;
  int len;
  segment(cu, seg, total, max_seqlen, beg, len);
  if (k0 >= len) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int krow = k0 + wave * 16 + c;
  const bool kvalid = krow < len;
  const half_t* seg_base = qkv + beg * rs + (int64_t)h * hs;
  const half_t* do_base = dout + beg * drs + (int64_t)h * dhs;
  h4 kf[ND], vf[ND];
  f4 dk[ND], dv[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    kf[kd] = vf[kd] = h4{0, 0, 0, 0};
    if (kvalid) {
      kf[kd] = ld4(seg_base + ss + (int64_t)krow * rs + kd * 16 + 4 * g);
      vf[kd] = ld4(seg_base + 2 * ss + (int64_t)krow * rs + kd * 16 + 4 * g);
    }
    dk[kd] = dv[kd] = f4{0.f, 0.f, 0.f, 0.f};
  }
  Staged<ND, NB> qst, ost;
  stage_load(qst, seg_base, rs, 0, len);
  stage_load(ost, do_base, drs, 0, len);
  for (int qb = 0; qb < len; qb += NB) {
    __syncthreads();
    stage_store<ND, NB, true, true>(qst, Qs, Qt);
    stage_store<ND, NB, true, true>(ost, Os, Ot);
    if (threadIdx.x < NB) {
      const int row = qb + threadIdx.x;
      const bool in = row < len;
      // +inf turns the probabilities of the rows beyond the segment into exp2(-inf) = 0
      Ls[threadIdx.x] = in ? lse[(int64_t)h * total + beg + row] * kLog2e : INFINITY;
      Ds[threadIdx.x] = in ? delta[(int64_t)h * total + beg + row] : 0.f;
    }
    __syncthreads();
    if (qb + NB < len) {
      stage_load(qst, seg_base, rs, qb + NB, len);
      stage_load(ost, do_base, drs, qb + NB, len);
    }
    const int nq = len - qb < NB ? len - qb : NB;
    for (int t0 = 0; t0 < nq; t0 += 16) {
      f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) {
        s = mfma(ld4(Qs + (t0 + c) * T::KS + kd * 16 + 4 * g), kf[kd], s);
        dp = mfma(ld4(Os + (t0 + c) * T::KS + kd * 16 + 4 * g), vf[kd], dp);
      }
      const f4 l2 = *reinterpret_cast<const f4*>(Ls + t0 + 4 * g);
      const f4 dl = *reinterpret_cast<const f4*>(Ds + t0 + 4 * g);
      f4 p, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = ex2(__builtin_fmaf(s[r], sl2, -l2[r]));
        ds[r] = p[r] * (dp[r] - dl[r]);
      }
      const h4 ph = to_half(p), dsh = to_half(ds);
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) {
        dv[kd] = mfma(ld4(Ot + (kd * 16 + c) * T::VS + t0 + 4 * g), ph, dv[kd]);
        dk[kd] = mfma(ld4(Qt + (kd * 16 + c) * T::VS + t0 + 4 * g), dsh, dk[kd]);
      }
    }
  }
  if (kvalid) {
    half_t* drow = dqkv + ((beg + krow) * 3 * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) {
      *reinterpret_cast<h4*>(drow + (int64_t)heads * D + kd * 16 + 4 * g) = to_half(dk[kd] * scale);
      *reinterpret_cast<h4*>(drow + 2 * (int64_t)heads * D + kd * 16 + 4 * g) = to_half(dv[kd]);
    }
  }
}

// dQ: a wave owns 16 queries (Q, dO fragments, log-sum-exp and delta in registers) and streams the keys.
template <int ND>
__global__ __launch_bounds__(kThreads) void k_backward_q(const half_t* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                         const half_t* __restrict__ dout, int64_t drs, int64_t dhs,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                         int qblocks, float sl2, float scale, half_t* __restrict__ dqkv,
                                                         int heads) {
  constexpr int NB = 128;
  typedef Tile<ND, NB> T;
  constexpr int D = T::D;
  __shared__ __align__(16) half_t Ks[NB * T::KS];
  __shared__ __align__(16) half_t Kt[D * T::VS];
  __shared__ __align__(16) half_t Vs[NB * T::KS];
  const int64_t seg = blockIdx.x / qblocks;
  const int q0 = (int)(blockIdx.x % qblocks) * kRowsPerGroup;
  const int h = blockIdx.z;
  int64_t beg;
  int len;
  segment(cu, seg, total, max_seqlen, beg, len);
  if (q0 >= len) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qrow = q0 + wave * 16 + c;
  const bool qvalid = qrow < len;
  const half_t* seg_base = qkv + beg * rs + (int64_t)h * hs;
  h4 qf[ND], of[ND];
  f4 dq[ND];
  float l2 = 0.f, dl = 0.f;
  if (qvalid) {
    l2 = lse[(int64_t)h * total + beg + qrow] * kLog2e;
    dl = delta[(int64_t)h * total + beg + qrow];
  }
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    qf[kd] = of[kd] = h4{0, 0, 0, 0};
    if (qvalid) {
      qf[kd] = ld4(seg_base + (int64_t)qrow * rs + kd * 16 + 4 * g);
      of[kd] = ld4(dout + (beg + qrow) * drs + (int64_t)h * dhs + kd * 16 + 4 * g);
    }
    dq[kd] = f4{0.f, 0.f, 0.f, 0.f};
  }
  Staged<ND, NB> kst, vst;
  stage_load(kst, seg_base + ss, rs, 0, len);
  stage_load(vst, seg_base + 2 * ss, rs, 0, len);
  for (int kb = 0; kb < len; kb += NB) {
    __syncthreads();
    stage_store<ND, NB, true, true>(kst, Ks, Kt);
    stage_store<ND, NB, true, false>(vst, Vs, nullptr);
    __syncthreads();
    if (kb + NB < len) {
      stage_load(kst, seg_base + ss, rs, kb + NB, len);
      stage_load(vst, seg_base + 2 * ss, rs, kb + NB, len);
    }
    const int nk = len - kb < NB ? len - kb : NB;
    for (int t0 = 0; t0 < nk; t0 += 16) {
      f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) {
        s = mfma(ld4(Ks + (t0 + c) * T::KS + kd * 16 + 4 * g), qf[kd], s);
        dp = mfma(ld4(Vs + (t0 + c) * T::KS + kd * 16 + 4 * g), of[kd], dp);
      }
      f4 ds;
      const bool whole = kb + t0 + 16 <= len;  // keys beyond the segment exist only in its last tile
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = ex2(__builtin_fmaf(s[r], sl2, -l2));
        if (!whole && kb + t0 + 4 * g + r >= len) p = 0.f;
        ds[r] = p * (dp[r] - dl);
      }
      const h4 dsh = to_half(ds);
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) dq[kd] = mfma(ld4(Kt + (kd * 16 + c) * T::VS + t0 + 4 * g), dsh, dq[kd]);
    }
  }
  if (qvalid) {
    half_t* drow = dqkv + ((beg + qrow) * 3 * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) *reinterpret_cast<h4*>(drow + kd * 16 + 4 * g) = to_half(dq[kd] * scale);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
constexpr int64_t kMaxRows = (int64_t)1 << 31;

bool stride_ok(int64_t s) { return s > 0 && s % 8 == 0; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Shape checks shared by every entry point; 0 when fine.
int check_shape(const char* who, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim, int64_t max_seqlen,
                float scale) {
  const std::string w(who);
  if (total < 0 || total >= kMaxRows) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": total out of range");
  if (nseg < 0 || nseg >= kMaxRows) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": nseg out of range");
  if (heads <= 0 || heads > 65535) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": heads must be in 1..65535");
  if (head_dim != 16 && head_dim != 32 && head_dim != 64)
    return fail(GCA_ERR_INVALID_ARGUMENT, w + ": head_dim must be 16, 32 or 64");
  if (max_seqlen < 0) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": max_seqlen is negative");
  if (!std::isfinite(scale)) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": softmax_scale is not finite");
  return 0;
}

// Workgroups per head: one per (segment, 64-row group of its first min(max_seqlen, total) rows).
int grid_of(const char* who, int64_t nseg, int64_t total, int64_t max_seqlen, int* groups, unsigned* blocks) {
  const int64_t rows = max_seqlen < total ? max_seqlen : total;
  const int64_t per = (rows + kRowsPerGroup - 1) / kRowsPerGroup;
  if (per * nseg >= kMaxRows)
    return fail(GCA_ERR_INVALID_ARGUMENT, std::string(who) + ": nseg * ceil(max_seqlen / 64) does not fit one grid");
  *groups = (int)per;
  *blocks = (unsigned)(per * nseg);
  return 0;
}

}  // namespace

extern "C" {

int gca_abi_version(void) { return GCA_ABI_VERSION; }
const char* gca_last_error(void) { return g_err.c_str(); }

size_t gca_lse_bytes(int64_t total, int32_t heads) {
  g_err.clear();
  if (total < 0 || total >= kMaxRows) return (size_t)(fail(0, "gca_lse_bytes: total out of range"));
  if (heads <= 0 || heads > 65535) return (size_t)(fail(0, "gca_lse_bytes: heads must be in 1..65535"));
  return (size_t)total * (size_t)heads * sizeof(float);
}

size_t gca_backward_workspace_bytes(int64_t total, int32_t heads) {
  g_err.clear();
  if (total < 0 || total >= kMaxRows) return (size_t)(fail(0, "gca_backward_workspace_bytes: total out of range"));
  if (heads <= 0 || heads > 65535) return (size_t)(fail(0, "gca_backward_workspace_bytes: heads must be in 1..65535"));
  return (size_t)total * (size_t)heads * sizeof(float);  // delta [heads][total]
}

int gca_varlen_forward(const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                       const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim,
                       int64_t max_seqlen, float softmax_scale, void* out, float* lse, void* hip_stream) {
  const char* who = "gca_varlen_forward";
  if (int rc = check_shape(who, nseg, total, heads, head_dim, max_seqlen, softmax_scale)) return rc;
  if (total == 0) return GCA_OK;
  if (!qkv || !out || !lse) return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_forward: null qkv, out or lse");
  if (!cu_seqlens) return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_forward: null cu_seqlens");
  if (!stride_ok(row_stride) || !stride_ok(slot_stride) || !stride_ok(head_stride))
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_forward: strides must be positive multiples of 8 elements");
  if (!aligned16(qkv) || !aligned16(out))
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_forward: qkv and out must be 16-byte aligned");
  int groups;
  unsigned blocks;
  if (int rc = grid_of(who, nseg, total, max_seqlen, &groups, &blocks)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)total * heads * head_dim * sizeof(half_t), st), "forward clear out");
  HIP_TRY(hipMemsetAsync(lse, 0, (size_t)total * heads * sizeof(float), st), "forward clear lse");
  if (blocks == 0) return GCA_OK;
  const float sl2 = softmax_scale * kLog2e;
  const dim3 grid(blocks, 1, (unsigned)heads);
#define GCA_FWD(ND)                                                                                                   \
  k_forward<ND><<<grid, kThreads, 0, st>>>((const half_t*)qkv, row_stride, slot_stride, head_stride, cu_seqlens, total, \
                                           (int)(max_seqlen < total ? max_seqlen : total), groups, sl2, (half_t*)out,   \
                                           lse, heads)
  if (head_dim == 16) GCA_FWD(1);
  else if (head_dim == 32) GCA_FWD(2);
  else GCA_FWD(4);
#undef GCA_FWD
  HIP_TRY(hipGetLastError(), "forward launch");
  return GCA_OK;
}

int gca_varlen_backward(const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                        const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride,
                        const float* lse, const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads,
                        int32_t head_dim, int64_t max_seqlen, float softmax_scale, void* dqkv, void* workspace,
                        size_t workspace_bytes, void* hip_stream) {
  const char* who = "gca_varlen_backward";
  if (int rc = check_shape(who, nseg, total, heads, head_dim, max_seqlen, softmax_scale)) return rc;
  if (total == 0) return GCA_OK;
  if (!qkv || !out || !dout || !lse || !dqkv)
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_backward: null qkv, out, dout, lse or dqkv");
  if (!cu_seqlens) return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_backward: null cu_seqlens");
  if (!stride_ok(row_stride) || !stride_ok(slot_stride) || !stride_ok(head_stride) || !stride_ok(dout_row_stride) ||
      !stride_ok(dout_head_stride))
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_backward: strides must be positive multiples of 8 elements");
  if (!aligned16(qkv) || !aligned16(out) || !aligned16(dout) || !aligned16(dqkv))
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_backward: qkv, out, dout and dqkv must be 16-byte aligned");
  const size_t need = (size_t)total * (size_t)heads * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(GCA_ERR_INVALID_ARGUMENT, "gca_varlen_backward: workspace is null or smaller than gca_backward_workspace_bytes");
  int groups;
  unsigned blocks;
  if (int rc = grid_of(who, nseg, total, max_seqlen, &groups, &blocks)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(dqkv, 0, (size_t)total * 3 * heads * head_dim * sizeof(half_t), st), "backward clear dqkv");
  if (blocks == 0) return GCA_OK;
  float* delta = (float*)workspace;
  const float sl2 = softmax_scale * kLog2e;
  const int mx = (int)(max_seqlen < total ? max_seqlen : total);
  const dim3 grid(blocks, 1, (unsigned)heads);
  const unsigned dblocks = (unsigned)(((int64_t)total * heads + kThreads - 1) / kThreads);
#define GCA_BWD(ND)                                                                                                     \
  do {                                                                                                                  \
    k_delta<ND><<<dblocks, kThreads, 0, st>>>((const half_t*)out, (const half_t*)dout, dout_row_stride,                 \
                                              dout_head_stride, total, heads, delta);                                   \
    k_backward_kv<ND><<<grid, kThreads, 0, st>>>((const half_t*)qkv, row_stride, slot_stride, head_stride,              \
                                                 (const half_t*)dout, dout_row_stride, dout_head_stride, lse, delta,    \
                                                 cu_seqlens, total, mx, groups, sl2, softmax_scale, (half_t*)dqkv,      \
                                                 heads);                                                                \
    k_backward_q<ND><<<grid, kThreads, 0, st>>>((const half_t*)qkv, row_stride, slot_stride, head_stride,               \
                                                (const half_t*)dout, dout_row_stride, dout_head_stride, lse, delta,     \
                                                cu_seqlens, total, mx, groups, sl2, softmax_scale, (half_t*)dqkv,       \
                                                heads);                                                                 \
  } while (0)
  if (head_dim == 16) GCA_BWD(1);
  else if (head_dim == 32) GCA_BWD(2);
  else GCA_BWD(4);
#undef GCA_BWD
  HIP_TRY(hipGetLastError(), "backward launch");
  return GCA_OK;
}

}  // extern "C"
