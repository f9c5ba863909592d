// gca_attention.hip -- MI355X (gfx950) kernels + C ABI (include/gca.h) of the point backbone's attention:
// variable-length, packed-QKV, non-causal softmax attention, in binary16 (flash_attn_varlen_qkvpacked_func) and in
// float32 (the backbone's non-flash branch).  DESIGN.md section 16.
//
// One set of kernels over the element type E.  A product over 16 values of k is
//   binary16  one v_mfma_f32_16x16x16_f16 (fp32 accumulation);
//   float32   four chained v_mfma_f32_16x16x4_f32 (a k-ordered fp32 fmaf chain), step j taking element j of the same
//             fragments: the instruction's own k slot g then stands for k = 4g + j in A and in B alike.
// So both types share the operand maps, lane l, c = l & 15, g = l >> 4:
//   A[row c][k 4g + j], B[k 4g + j][col c] (j = 0..3, one fragment of 8 or 16 bytes), C/D[row 4g + r][col c] (r = 0..3).
// A C/D tile is therefore already the B fragment of a following product that sums over the tile's ROW index, and
// the orientation of every first product is chosen for that:
//   forward   S^T = K Q^T  (key on the register, query on the lane)   ->  O^T += V^T P^T
//   dQ pass   S^T = K Q^T, dP^T = V dO^T, dS^T                        ->  dQ^T += K^T dS^T
//   dK/dV     S = Q K^T, dP = dO V^T (query on the register, key on the lane) -> dV^T += dO^T P, dK^T += Q^T dS
// so neither P nor dS ever passes through LDS, and every result tile has four consecutive channels of one row
// on a lane (one 8- or 16-byte store).  The operand that stays (Q and dO of a query tile; K and V of a key tile) lives
// in registers; the streamed one is staged in LDS in blocks, row-major for the fragments read by rows and
// transposed for those read by columns, at the conflict-free pitches of Tile.
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

// float32: the same fragments, four floats of consecutive k on a lane, through four steps of the f32-input MFMA.
__device__ __forceinline__ f4 mfma(f4 a, f4 b, f4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
  return c;
}
__device__ __forceinline__ f4 ld4(const float* p) { return *reinterpret_cast<const f4*>(p); }

// The element type: its fragment, the elements of one 16-byte piece, the conversion of an fp32 tile to an operand or a
// result (none for float32: P, dS, out and dqkv stay fp32), and the units of the exponent.  The kernels get ONE score
// factor `sc` and turn a raw score s into the exponent s * sc; expo() is exp of a difference of two exponents, lse() what
// the forward stores from the running maximum m and the row sum l, row_lse() what the backward subtracts, prob() the
// probability of a raw score.
//   binary16  sc = scale log2(e): exponents in units of log2, exp is v_exp_f32 itself; the stored natural logarithm is
//             converted back by one fp32 product.  2^-24 |lse| is far below the 2^-11 of the operand P.
//   float32   sc = scale: exponents in natural units, so that the stored log-sum-exp IS the forward's own quantity (the
//             logarithm of l runs in double, once per row, and the sum is rounded once) and the backward subtracts it
//             from the same fp32 product s * scale the forward formed: where one key holds all the weight the difference
//             is exactly 0 and P exactly 1.  |lse| is about log(keys) even where every score is tiny, so the fp32
//             rounding of a - lse and of its product with log2(e) would cost P several 2^-24 that the scores do not
//             explain: both rounding errors are computed (two-sum; fma) and applied, P = exp2(hi) (1 + lo ln 2 + r).
constexpr float kLog2eLo = (float)(1.4426950408889634 - (double)1.4426950408889634f);  // log2(e) - kLog2e
template <typename E>
struct Elem;
template <>
struct Elem<half_t> {
  typedef h4 frag;
  static constexpr int PIECE = 8;
  static __device__ __forceinline__ h4 from(f4 v) { return to_half(v); }
  static __host__ __device__ __forceinline__ float factor(float scale) { return scale * kLog2e; }
  static __device__ __forceinline__ float expo(float x) { return ex2(x); }
  static __device__ __forceinline__ float lse(float m, float l) { return (m + log2f(l)) * kLn2; }
  static __device__ __forceinline__ float row_lse(float lse) { return lse * kLog2e; }
  static __device__ __forceinline__ float prob(float s, float sc, float L) { return ex2(__builtin_fmaf(s, sc, -L)); }
};
template <>
struct Elem<float> {
  typedef f4 frag;
  static constexpr int PIECE = 4;
  static __device__ __forceinline__ f4 from(f4 v) { return v; }
  static __host__ __device__ __forceinline__ float factor(float scale) { return scale; }
  static __device__ __forceinline__ float expo(float x) { return ex2(x * kLog2e); }
  static __device__ __forceinline__ float lse(float m, float l) { return (float)((double)m + log((double)l)); }
  static __device__ __forceinline__ float row_lse(float lse) { return lse; }
  static __device__ __forceinline__ float prob(float s, float sc, float L) {
    const float a = s * sc;
    const float t = a - L, bb = t - a;
    const float r = (a - (t - bb)) + (-L - bb);  // a - L = t + r
    const float hi = t * kLog2e;
    const float lo = __builtin_fmaf(t, kLog2e, -hi) + t * kLog2eLo;  // t log2(e) = hi + lo
    const float e = ex2(hi);
    return __builtin_fmaf(e, __builtin_fmaf(lo, kLn2, r), e);
  }
};

// Pitches of the LDS images, in elements.  binary16 (8-byte fragment reads): row-major D + 4 halves, transposed
// NB + 16 halves = 72 / 40 words = 8 mod 64 / 40 mod 64.  float32 (16-byte fragment reads, which the LDS serves in
// groups of 16 lanes -- 8 values of c at one g and 8 at the next): a pitch of 8 mod 16 words puts the 16 fragments of
// a group on 16 different quads of banks, so row-major D + 8 and transposed NB + 8 words.
template <typename E, int ND, int NB>
struct Tile {
  static constexpr int D = 16 * ND;
  static constexpr int KS = sizeof(E) == 4 ? D + 8 : (ND == 1 ? 16 : D + 4);
  static constexpr int VS = sizeof(E) == 4 ? NB + 8 : NB + 16;
};

// Rows per staged block: 128, less where the float32 images (twice the bytes) would not leave 64 KB of LDS to a
// workgroup.  FWD serves the forward and the dQ pass (keys), KV the dK / dV pass (queries).
template <typename E, int ND>
struct Block {
  static constexpr int FWD = sizeof(E) == 4 && ND == 4 ? 64 : 128;
  static constexpr int KV = sizeof(E) == 4 ? (ND == 1 ? 128 : ND == 2 ? 64 : 32) : (ND <= 2 ? 128 : 64);
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
template <typename E, int ND, int NB>
struct Staged {
  static constexpr int CPR = 16 * ND / Elem<E>::PIECE;                   // 16-byte pieces per row
  static constexpr int N = (NB * CPR + kThreads - 1) / kThreads;         // pieces per thread
  u4 v[N];
};

template <typename E, int ND, int NB>
__device__ __forceinline__ void stage_load(Staged<E, ND, NB>& st, const E* base, int64_t rs, int r0, int len) {
  typedef Staged<E, ND, NB> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) {
    const int idx = threadIdx.x + i * kThreads;
    const int row = idx / S::CPR, cc = idx % S::CPR;
    st.v[i] = u4{0u, 0u, 0u, 0u};
    if (idx < NB * S::CPR && r0 + row < len)
      st.v[i] = *reinterpret_cast<const u4*>(base + (int64_t)(r0 + row) * rs + cc * Elem<E>::PIECE);
  }
}

template <int ND, int NB, bool ROW, bool TR>
__device__ __forceinline__ void stage_store(const Staged<half_t, ND, NB>& st, half_t* Xs, half_t* Xt) {
  typedef Tile<half_t, ND, NB> T;
  typedef Staged<half_t, ND, NB> S;
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

template <int ND, int NB, bool ROW, bool TR>
__device__ __forceinline__ void stage_store(const Staged<float, ND, NB>& st, float* Xs, float* Xt) {
  typedef Tile<float, ND, NB> T;
  typedef Staged<float, ND, NB> S;
#pragma unroll
  for (int i = 0; i < S::N; ++i) {
    const int idx = threadIdx.x + i * kThreads;
    if (idx >= NB * S::CPR) break;
    const int row = idx / S::CPR, cc = idx % S::CPR;
    const u4 v = st.v[i];
    if (ROW) *reinterpret_cast<u4*>(Xs + row * T::KS + cc * 4) = v;
    if (TR) {
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) reinterpret_cast<unsigned*>(Xt)[(cc * 4 + j) * T::VS + row] = w[j];
    }
  }
}

// Two-level sums of the float32 path.  A result tile sums over every row of the segment; as ONE fp32 chain its rounding
// error grows with the square root of the rows times the size of the partial sums (measured: 5 float32 units in dV at
// 300 rows of near-uniform attention, 3 x the torch formulation at 1300).  So the float32 kernels sum kPartialRows rows
// at a time from zero and add each such partial to the running tile.  binary16 keeps its single chain: its error is the
// 2^-11 of the operands, and its bits are pinned.
constexpr int kPartialRows = 64;
template <int ND>
__device__ __forceinline__ void clear(f4 (&t)[ND]) {
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) t[kd] = f4{0.f, 0.f, 0.f, 0.f};
}
template <int ND>
__device__ __forceinline__ void add(f4 (&total)[ND], const f4 (&part)[ND]) {
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) total[kd] = total[kd] + part[kd];
}

// ---- forward ---------------------------------------------------------------------------------------------------
// 64 keys (LDS rows c0 .. c0 + 63) against the wave's 16 queries: S^T tiles, running maximum `m` (in the units of
// Elem<E>, shared by the four lanes of a query), per-lane partial row sums `lv`, O^T += V^T P^T.  MASK: only the
// first `valid` keys are inside the segment.  float32 sums the step's 64 keys from zero and adds that to the running
// tile (Partial below); binary16 continues the running tile.
template <typename E, int ND, int NB, bool MASK>
__device__ __forceinline__ void forward_step(const E* Ks, const E* Vt, const typename Elem<E>::frag (&qf)[ND], f4 (&o)[ND],
                                             float& m, f4& lv, float sc, int c0, int c, int g, int valid) {
  typedef Tile<E, ND, NB> T;
  f4 s[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    s[t] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) s[t] = mfma(ld4(Ks + (c0 + t * 16 + c) * T::KS + kd * 16 + 4 * g), qf[kd], s[t]);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    s[t] = s[t] * sc;
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
  const float alpha = Elem<E>::expo(m - mn);
  m = mn;
  lv = lv * alpha;
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) o[kd] = o[kd] * alpha;
  constexpr bool F32 = sizeof(E) == 4;
  f4 part[F32 ? ND : 1];  // float32: the step's own sum
  if (F32) clear(part);
  f4* acc = F32 ? part : o;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f4 e = s[t] - mn;
    f4 p;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = Elem<E>::expo(e[r]);
    lv = lv + p;
    const typename Elem<E>::frag ph = Elem<E>::from(p);
#pragma unroll
    for (int kd = 0; kd < ND; ++kd)
      acc[kd] = mfma(ld4(Vt + (kd * 16 + c) * T::VS + c0 + t * 16 + 4 * g), ph, acc[kd]);
  }
  if constexpr (F32) add(o, part);
}

template <typename E, int ND>
__global__ __launch_bounds__(kThreads) void k_forward(const E* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                      const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                      int qblocks, float sc, E* __restrict__ out,
                                                      float* __restrict__ lse, int heads) {
  constexpr int NB = Block<E, ND>::FWD;
  typedef Tile<E, ND, NB> T;
  typedef typename Elem<E>::frag frag;
  constexpr int D = T::D;
  __shared__ __align__(16) E Ks[NB * T::KS];
  __shared__ __align__(16) E Vt[D * T::VS];
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
  const E* seg_base = qkv + beg * rs + (int64_t)h * hs;
  frag qf[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    qf[kd] = frag{0, 0, 0, 0};
    if (qvalid) qf[kd] = ld4(seg_base + (int64_t)qrow * rs + kd * 16 + 4 * g);
  }
  f4 o[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) o[kd] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY;
  f4 lv = {0.f, 0.f, 0.f, 0.f};

  Staged<E, ND, NB> kst, vst;
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
        forward_step<E, ND, NB, false>(Ks, Vt, qf, o, m, lv, sc, c0, c, g, 64);
      else
        forward_step<E, ND, NB, true>(Ks, Vt, qf, o, m, lv, sc, c0, c, g, nk - c0);
    }
  }
  float l = (lv[0] + lv[1]) + (lv[2] + lv[3]);
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qvalid) {
    E* orow = out + ((beg + qrow) * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) {
      f4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = o[kd][r] / l;
      *reinterpret_cast<frag*>(orow + kd * 16 + 4 * g) = Elem<E>::from(v);
    }
    if (g == 0) lse[(int64_t)h * total + beg + qrow] = Elem<E>::lse(m, l);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------
// delta[h][row] = sum_c dout[row][h][c] * out[row][h][c], fp32, channels in order.
template <typename E, int ND>
__global__ __launch_bounds__(kThreads) void k_delta(const E* __restrict__ out, const E* __restrict__ dout,
                                                    int64_t drs, int64_t dhs, int64_t total, int heads,
                                                    float* __restrict__ delta) {
  constexpr int D = 16 * ND;
  const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total * heads) return;
  const int64_t row = idx / heads;
  const int h = (int)(idx % heads);
  constexpr int PIECE = Elem<E>::PIECE;
  const E* o = out + idx * D;
  const E* d = dout + row * drs + (int64_t)h * dhs;
  float acc = 0.f;
#pragma unroll
  for (int cc = 0; cc < D / PIECE; ++cc) {
    const u4 a = *reinterpret_cast<const u4*>(o + cc * PIECE), b = *reinterpret_cast<const u4*>(d + cc * PIECE);
    const E* ah = reinterpret_cast<const E*>(&a);
    const E* bh = reinterpret_cast<const E*>(&b);
#pragma unroll
    for (int i = 0; i < PIECE; ++i) acc += (float)ah[i] * (float)bh[i];
  }
  delta[(int64_t)h * total + row] = acc;
}

// dK, dV: a wave owns 16 keys (K, V fragments in registers) and streams the segment's queries through LDS.
template <typename E, int ND>
__global__ __launch_bounds__(kThreads) void k_backward_kv(const E* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                          const E* __restrict__ dout, int64_t drs, int64_t dhs,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                          int kblocks, float sc, float scale, E* __restrict__ dqkv,
                                                          int heads) {
  // queries per staged block (LDS at d = 16 / 32 / 64: binary16 19 / 37 / 38 KB, float32 42 / 39 / 39 KB)
  constexpr int NB = Block<E, ND>::KV;
  typedef Tile<E, ND, NB> T;
  typedef typename Elem<E>::frag frag;
  constexpr int D = T::D;
  __shared__ __align__(16) E Qs[NB * T::KS];
  __shared__ __align__(16) E Qt[D * T::VS];
  __shared__ __align__(16) E Os[NB * T::KS];
  __shared__ __align__(16) E Ot[D * T::VS];
  constexpr bool F32 = sizeof(E) == 4;
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
  const E* seg_base = qkv + beg * rs + (int64_t)h * hs;
  const E* do_base = dout + beg * drs + (int64_t)h * dhs;
  frag kf[ND], vf[ND];
  f4 dk[ND], dv[ND];
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    kf[kd] = vf[kd] = frag{0, 0, 0, 0};
    if (kvalid) {
      kf[kd] = ld4(seg_base + ss + (int64_t)krow * rs + kd * 16 + 4 * g);
      vf[kd] = ld4(seg_base + 2 * ss + (int64_t)krow * rs + kd * 16 + 4 * g);
    }
    dk[kd] = dv[kd] = f4{0.f, 0.f, 0.f, 0.f};
  }
  Staged<E, ND, NB> qst, ost;
  stage_load(qst, seg_base, rs, 0, len);
  stage_load(ost, do_base, drs, 0, len);
  for (int qb = 0; qb < len; qb += NB) {
    __syncthreads();
    stage_store<ND, NB, true, true>(qst, Qs, Qt);
    stage_store<ND, NB, true, true>(ost, Os, Ot);
    if (threadIdx.x < NB) {
      const int row = qb + threadIdx.x;
      const bool in = row < len;
      // binary16: +inf turns the probabilities of the rows beyond the segment into exp2(-inf) = 0; float32 (whose
      // prob() would make inf - inf of it) clears them below
      Ls[threadIdx.x] = in ? Elem<E>::row_lse(lse[(int64_t)h * total + beg + row]) : (F32 ? 0.f : INFINITY);
      Ds[threadIdx.x] = in ? delta[(int64_t)h * total + beg + row] : 0.f;
    }
    __syncthreads();
    if (qb + NB < len) {
      stage_load(qst, seg_base, rs, qb + NB, len);
      stage_load(ost, do_base, drs, qb + NB, len);
    }
    const int nq = len - qb < NB ? len - qb : NB;
    auto tile = [&](int t0, f4(&adv)[ND], f4(&adk)[ND]) {  // 16 queries against the wave's keys, into adv and adk
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
        p[r] = Elem<E>::prob(s[r], sc, l2[r]);
        if (F32 && t0 + 4 * g + r >= nq) p[r] = 0.f;
        ds[r] = p[r] * (dp[r] - dl[r]);
      }
      const frag ph = Elem<E>::from(p), dsh = Elem<E>::from(ds);
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) {
        adv[kd] = mfma(ld4(Ot + (kd * 16 + c) * T::VS + t0 + 4 * g), ph, adv[kd]);
        adk[kd] = mfma(ld4(Qt + (kd * 16 + c) * T::VS + t0 + 4 * g), dsh, adk[kd]);
      }
    };
    if constexpr (F32) {
      for (int p0 = 0; p0 < nq; p0 += kPartialRows) {
        f4 pv[ND], pk[ND];
        clear(pv);
        clear(pk);
        for (int t0 = p0; t0 < nq && t0 < p0 + kPartialRows; t0 += 16) tile(t0, pv, pk);
        add(dv, pv);
        add(dk, pk);
      }
    } else {
      for (int t0 = 0; t0 < nq; t0 += 16) tile(t0, dv, dk);
    }
  }
  if (kvalid) {
    E* drow = dqkv + ((beg + krow) * 3 * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) {
      *reinterpret_cast<frag*>(drow + (int64_t)heads * D + kd * 16 + 4 * g) = Elem<E>::from(dk[kd] * scale);
      *reinterpret_cast<frag*>(drow + 2 * (int64_t)heads * D + kd * 16 + 4 * g) = Elem<E>::from(dv[kd]);
    }
  }
}

// dQ: a wave owns 16 queries (Q, dO fragments, log-sum-exp and delta in registers) and streams the keys.
template <typename E, int ND>
__global__ __launch_bounds__(kThreads) void k_backward_q(const E* __restrict__ qkv, int64_t rs, int64_t ss, int64_t hs,
                                                         const E* __restrict__ dout, int64_t drs, int64_t dhs,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         const int32_t* __restrict__ cu, int64_t total, int max_seqlen,
                                                         int qblocks, float sc, float scale, E* __restrict__ dqkv,
                                                         int heads) {
  constexpr int NB = Block<E, ND>::FWD;
  typedef Tile<E, ND, NB> T;
  typedef typename Elem<E>::frag frag;
  constexpr int D = T::D;
  __shared__ __align__(16) E Ks[NB * T::KS];
  __shared__ __align__(16) E Kt[D * T::VS];
  __shared__ __align__(16) E Vs[NB * T::KS];
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
  const E* seg_base = qkv + beg * rs + (int64_t)h * hs;
  frag qf[ND], of[ND];
  f4 dq[ND];
  float l2 = 0.f, dl = 0.f;
  if (qvalid) {
    l2 = Elem<E>::row_lse(lse[(int64_t)h * total + beg + qrow]);
    dl = delta[(int64_t)h * total + beg + qrow];
  }
#pragma unroll
  for (int kd = 0; kd < ND; ++kd) {
    qf[kd] = of[kd] = frag{0, 0, 0, 0};
    if (qvalid) {
      qf[kd] = ld4(seg_base + (int64_t)qrow * rs + kd * 16 + 4 * g);
      of[kd] = ld4(dout + (beg + qrow) * drs + (int64_t)h * dhs + kd * 16 + 4 * g);
    }
    dq[kd] = f4{0.f, 0.f, 0.f, 0.f};
  }
  Staged<E, ND, NB> kst, vst;
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
    auto tile = [&](int t0, f4(&adq)[ND]) {  // 16 keys against the wave's queries, into adq
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
        float p = Elem<E>::prob(s[r], sc, l2);
        if (!whole && kb + t0 + 4 * g + r >= len) p = 0.f;
        ds[r] = p * (dp[r] - dl);
      }
      const frag dsh = Elem<E>::from(ds);
#pragma unroll
      for (int kd = 0; kd < ND; ++kd) adq[kd] = mfma(ld4(Kt + (kd * 16 + c) * T::VS + t0 + 4 * g), dsh, adq[kd]);
    };
    if constexpr (sizeof(E) == 4) {
      for (int p0 = 0; p0 < nk; p0 += kPartialRows) {
        f4 pq[ND];
        clear(pq);
        for (int t0 = p0; t0 < nk && t0 < p0 + kPartialRows; t0 += 16) tile(t0, pq);
        add(dq, pq);
      }
    } else {
      for (int t0 = 0; t0 < nk; t0 += 16) tile(t0, dq);
    }
  }
  if (qvalid) {
    E* drow = dqkv + ((beg + qrow) * 3 * heads + h) * (int64_t)D;
#pragma unroll
    for (int kd = 0; kd < ND; ++kd) *reinterpret_cast<frag*>(drow + kd * 16 + 4 * g) = Elem<E>::from(dq[kd] * scale);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
constexpr int64_t kMaxRows = (int64_t)1 << 31;

// a strided operand: strides are positive multiples of one 16-byte piece (8 halves, 4 floats)
template <typename E>
bool stride_ok(int64_t s) { return s > 0 && s % Elem<E>::PIECE == 0; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
template <typename E>
std::string stride_rule(const std::string& who) {
  return who + ": strides must be positive multiples of " + std::to_string(Elem<E>::PIECE) + " elements";
}

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

// The forward of either element type, for the entry point `who`.
template <typename E>
int forward(const char* who, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
            const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim, int64_t max_seqlen,
            float softmax_scale, void* out, float* lse, void* hip_stream) {
  const std::string w(who);
  if (int rc = check_shape(who, nseg, total, heads, head_dim, max_seqlen, softmax_scale)) return rc;
  if (total == 0) return GCA_OK;
  if (!qkv || !out || !lse) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": null qkv, out or lse");
  if (!cu_seqlens) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": null cu_seqlens");
  if (!stride_ok<E>(row_stride) || !stride_ok<E>(slot_stride) || !stride_ok<E>(head_stride))
    return fail(GCA_ERR_INVALID_ARGUMENT, stride_rule<E>(w));
  if (!aligned16(qkv) || !aligned16(out))
    return fail(GCA_ERR_INVALID_ARGUMENT, w + ": qkv and out must be 16-byte aligned");
  int groups;
  unsigned blocks;
  if (int rc = grid_of(who, nseg, total, max_seqlen, &groups, &blocks)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)total * heads * head_dim * sizeof(E), st), "forward clear out");
  HIP_TRY(hipMemsetAsync(lse, 0, (size_t)total * heads * sizeof(float), st), "forward clear lse");
  if (blocks == 0) return GCA_OK;
  const float sc = Elem<E>::factor(softmax_scale);  // the kernels' score factor, in the units of Elem<E>
  const dim3 grid(blocks, 1, (unsigned)heads);
#define GCA_FWD(ND)                                                                                                \
  k_forward<E, ND><<<grid, kThreads, 0, st>>>((const E*)qkv, row_stride, slot_stride, head_stride, cu_seqlens, total, \
                                              (int)(max_seqlen < total ? max_seqlen : total), groups, sc, (E*)out,  \
                                              lse, heads)
  if (head_dim == 16) GCA_FWD(1);
  else if (head_dim == 32) GCA_FWD(2);
  else GCA_FWD(4);
#undef GCA_FWD
  HIP_TRY(hipGetLastError(), "forward launch");
  return GCA_OK;
}

template <typename E>
int backward(const char* who, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
             const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride, const float* lse,
             const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim, int64_t max_seqlen,
             float softmax_scale, void* dqkv, void* workspace, size_t workspace_bytes, void* hip_stream) {
  const std::string w(who);
  if (int rc = check_shape(who, nseg, total, heads, head_dim, max_seqlen, softmax_scale)) return rc;
  if (total == 0) return GCA_OK;
  if (!qkv || !out || !dout || !lse || !dqkv)
    return fail(GCA_ERR_INVALID_ARGUMENT, w + ": null qkv, out, dout, lse or dqkv");
  if (!cu_seqlens) return fail(GCA_ERR_INVALID_ARGUMENT, w + ": null cu_seqlens");
  if (!stride_ok<E>(row_stride) || !stride_ok<E>(slot_stride) || !stride_ok<E>(head_stride) ||
      !stride_ok<E>(dout_row_stride) || !stride_ok<E>(dout_head_stride))
    return fail(GCA_ERR_INVALID_ARGUMENT, stride_rule<E>(w));
  if (!aligned16(qkv) || !aligned16(out) || !aligned16(dout) || !aligned16(dqkv))
    return fail(GCA_ERR_INVALID_ARGUMENT, w + ": qkv, out, dout and dqkv must be 16-byte aligned");
  const size_t need = (size_t)total * (size_t)heads * sizeof(float);
  if (!workspace || workspace_bytes < need)
    return fail(GCA_ERR_INVALID_ARGUMENT, w + ": workspace is null or smaller than gca_backward_workspace_bytes");
  int groups;
  unsigned blocks;
  if (int rc = grid_of(who, nseg, total, max_seqlen, &groups, &blocks)) return rc;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipMemsetAsync(dqkv, 0, (size_t)total * 3 * heads * head_dim * sizeof(E), st), "backward clear dqkv");
  if (blocks == 0) return GCA_OK;
  float* delta = (float*)workspace;
  const float sc = Elem<E>::factor(softmax_scale);  // the kernels' score factor, in the units of Elem<E>
  const int mx = (int)(max_seqlen < total ? max_seqlen : total);
  const dim3 grid(blocks, 1, (unsigned)heads);
  const unsigned dblocks = (unsigned)(((int64_t)total * heads + kThreads - 1) / kThreads);
#define GCA_BWD(ND)                                                                                                   \
  do {                                                                                                                \
    k_delta<E, ND><<<dblocks, kThreads, 0, st>>>((const E*)out, (const E*)dout, dout_row_stride, dout_head_stride,    \
                                                 total, heads, delta);                                                \
    k_backward_kv<E, ND><<<grid, kThreads, 0, st>>>((const E*)qkv, row_stride, slot_stride, head_stride,              \
                                                    (const E*)dout, dout_row_stride, dout_head_stride, lse, delta,    \
                                                    cu_seqlens, total, mx, groups, sc, softmax_scale, (E*)dqkv,      \
                                                    heads);                                                           \
    k_backward_q<E, ND><<<grid, kThreads, 0, st>>>((const E*)qkv, row_stride, slot_stride, head_stride,               \
                                                   (const E*)dout, dout_row_stride, dout_head_stride, lse, delta,     \
                                                   cu_seqlens, total, mx, groups, sc, softmax_scale, (E*)dqkv,       \
                                                   heads);                                                            \
  } while (0)
  if (head_dim == 16) GCA_BWD(1);
  else if (head_dim == 32) GCA_BWD(2);
  else GCA_BWD(4);
#undef GCA_BWD
  HIP_TRY(hipGetLastError(), "backward launch");
  return GCA_OK;
}

}  // namespace

extern "C" {

int gca_abi_version(void) { return GCA_ABI_VERSION; }
const char* gca_last_error(void) { return g_err.c_str(); }
int gca_dtypes(void) { return 1 << GCA_F16 | 1 << GCA_F32; }

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
  return forward<half_t>("gca_varlen_forward", qkv, row_stride, slot_stride, head_stride, cu_seqlens, nseg, total, heads,
                         head_dim, max_seqlen, softmax_scale, out, lse, hip_stream);
}

int gca_varlen_backward(const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                        const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride,
                        const float* lse, const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads,
                        int32_t head_dim, int64_t max_seqlen, float softmax_scale, void* dqkv, void* workspace,
                        size_t workspace_bytes, void* hip_stream) {
  return backward<half_t>("gca_varlen_backward", qkv, row_stride, slot_stride, head_stride, out, dout, dout_row_stride,
                          dout_head_stride, lse, cu_seqlens, nseg, total, heads, head_dim, max_seqlen, softmax_scale, dqkv,
                          workspace, workspace_bytes, hip_stream);
}

int gca_varlen_forward_t(int dtype, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                         const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim,
                         int64_t max_seqlen, float softmax_scale, void* out, float* lse, void* hip_stream) {
  const char* who = "gca_varlen_forward_t";
  if (dtype == GCA_F16)
    return forward<half_t>(who, qkv, row_stride, slot_stride, head_stride, cu_seqlens, nseg, total, heads, head_dim,
                           max_seqlen, softmax_scale, out, lse, hip_stream);
  if (dtype == GCA_F32)
    return forward<float>(who, qkv, row_stride, slot_stride, head_stride, cu_seqlens, nseg, total, heads, head_dim,
                          max_seqlen, softmax_scale, out, lse, hip_stream);
  return fail(GCA_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown dtype (gca_dtypes() has the ones the library runs)");
}

int gca_varlen_backward_t(int dtype, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                          const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride,
                          const float* lse, const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads,
                          int32_t head_dim, int64_t max_seqlen, float softmax_scale, void* dqkv, void* workspace,
                          size_t workspace_bytes, void* hip_stream) {
  const char* who = "gca_varlen_backward_t";
  if (dtype == GCA_F16)
    return backward<half_t>(who, qkv, row_stride, slot_stride, head_stride, out, dout, dout_row_stride, dout_head_stride,
                            lse, cu_seqlens, nseg, total, heads, head_dim, max_seqlen, softmax_scale, dqkv, workspace,
                            workspace_bytes, hip_stream);
  if (dtype == GCA_F32)
    return backward<float>(who, qkv, row_stride, slot_stride, head_stride, out, dout, dout_row_stride, dout_head_stride,
                           lse, cu_seqlens, nseg, total, heads, head_dim, max_seqlen, softmax_scale, dqkv, workspace,
                           workspace_bytes, hip_stream);
  return fail(GCA_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown dtype (gca_dtypes() has the ones the library runs)");
}

}  // extern "C"
