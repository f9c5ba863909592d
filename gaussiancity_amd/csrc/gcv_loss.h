// gcv_loss.h -- K20 (L1, optionally masked), K21 (the N+1-label GAN loss) and K22 (the discriminator's label map) of
// libgcv_hip.so; included by gcv_points.hip, whose helpers (fail, HIP_TRY, misaligned) it uses.
// Reference behaviour: core/train.py:285 (L1Loss()(a * mask, b * mask)), losses/gan.py:55-97 (GANLoss.loss) and
// models/discriminator.py:177-189 (_smooth_interp: area interpolation, one-hot of the first maximal channel).
//
// None of this is bandwidth (the largest tensor of a training step is a few MB): the kernels exist to make one or two
// launches of what is a dozen torch kernels each.  They are written for that and for a fixed summation order:
//
//   partial sums   a workgroup of 256 threads takes L1_ITEMS / GAN_ITEMS consecutive items (elements for K20, pixels for
//                  K21) -- a function of the shape alone, never of the grid the device can hold.  A thread adds its items
//                  in ascending order (item = first + k * 256 + thread), the 64 lanes of a wave fold with __shfl_down
//                  (32, 16, ..., 1), the four wave sums go through LDS and thread 0 adds them in wave order.
//   fold           a second launch of ONE workgroup: thread t adds partials t, t + 256, ..., then the same shuffle / LDS
//                  tree, one division by the count, one rounding to float.
//   binary64 sums  every addition above is binary64, and so is a partial sum in memory: a float partial of 256 pixels
//                  would be rounded as coarsely as the loss itself, and the loss would carry two such roundings (a
//                  16 x 16 map is one partial: one float away from the nearest, where upstream's float32 is).  K20's terms are
//                  the float32 terms of the operator; K21's per-pixel log-sum-exp and softmax are evaluated in binary64
//                  from the float logits (a few thousand pixels: the cost does not show), so the loss is the float
//                  nearest to the binary64 value in all but boundary cases.
//   no atomics, no "last workgroup folds" inside the first launch: the two-launch form has no cross-XCD protocol to get
//                  wrong, and a kernel boundary is a microsecond or two.
//   backward       one launch that recomputes the term from the inputs and reads the incoming gradient from the device.
//   label map      one thread per output pixel, channels in ascending order, each channel's window in row-major order.
//
// The library is built with -ffp-contract=off: every product, difference and sum below is one rounding.
#pragma once

namespace {

constexpr int LOSS_MAX_CLASSES = 32;
constexpr int LOSS_BLOCK = 256;
constexpr int L1_PER_THREAD = 16;
constexpr int L1_ITEMS = LOSS_BLOCK * L1_PER_THREAD;  // elements per partial sum
constexpr int GAN_ITEMS = LOSS_BLOCK;                 // pixels per partial sum: one per thread

// The sum of `v` over a workgroup of LOSS_BLOCK threads, valid in thread 0.  `lds`: LOSS_BLOCK / 64 values.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    v = lds[0];
#pragma unroll
    for (int k = 1; k < LOSS_BLOCK / 64; k++) v += lds[k];
  }
  return v;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_loss_fold(const double* __restrict__ partials, unsigned n_partials,
                                                         double count, float* __restrict__ out) {
  __shared__ double lds[LOSS_BLOCK / 64];
  double acc = 0.0;
  for (unsigned i = threadIdx.x; i < n_partials; i += LOSS_BLOCK) acc += partials[i];
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) out[0] = (float)(acc / count);
}

// ---- K20 ---------------------------------------------------------------------------------------------------------
struct L1Args {
  const float *a, *b, *mask;  // mask: or null
  long long a_bs, a_cs, a_rs, b_bs, b_cs, b_rs, m_bs, m_rs;  // elements; the pixel stride is 1
  unsigned B, C, H, W, n;  // n = B * C * H * W < 2^31
};

// Element i of the logical [B][C][H][W] order: the term fl(fl(a m) - fl(b m)) (a - b without a mask) and the mask value.
__device__ __forceinline__ float l1_term(const L1Args& s, unsigned i, float& m) {
  const unsigned x = i % s.W, r = i / s.W, y = r % s.H, q = r / s.H, c = q % s.C, b = q / s.C;
  float av = s.a[b * s.a_bs + c * s.a_cs + y * s.a_rs + x];
  float bv = s.b[b * s.b_bs + c * s.b_cs + y * s.b_rs + x];
  m = 1.0f;
  if (s.mask) {
    m = s.mask[b * s.m_bs + y * s.m_rs + x];
    av = av * m;
    bv = bv * m;
  }
  return av - bv;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_l1_partials(const L1Args s, double* __restrict__ partials) {
  __shared__ double lds[LOSS_BLOCK / 64];
  const unsigned first = blockIdx.x * (unsigned)L1_ITEMS + threadIdx.x;
  double acc = 0.0;
  float m;
#pragma unroll 4
  for (int k = 0; k < L1_PER_THREAD; k++) {
    const unsigned i = first + (unsigned)k * LOSS_BLOCK;
    if (i < s.n) acc += (double)fabsf(l1_term(s, i, m));
  }
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// da = fl(fl(g / count) * sign(t)) * m, db = -da; contiguous [B][C][H][W], either may be null.
__global__ __launch_bounds__(LOSS_BLOCK) void k_l1_backward(const L1Args s, const float* __restrict__ g, double count,
                                                           float* __restrict__ da, float* __restrict__ db) {
  const unsigned i = blockIdx.x * (unsigned)LOSS_BLOCK + threadIdx.x;
  if (i >= s.n) return;
  float m;
  const float t = l1_term(s, i, m);
  const float scale = (float)((double)g[0] / count);  // the count is exact, as in the fold
  const float sg = t > 0.0f ? scale : (t < 0.0f ? -scale : 0.0f);  // sign(0) = 0; a NaN term gives 0 as well
  const float v = s.mask ? sg * m : sg;
  if (da) da[i] = v;
  if (db) db[i] = -v;
}

// ---- K21 ---------------------------------------------------------------------------------------------------------
struct GanArgs {
  const float *pred, *label, *weight;  // weight: or null
  long long p_bs, p_cs, p_rs, l_bs, l_cs, l_rs, w_bs, w_rs;  // elements; the pixel stride is 1
  unsigned B, C, H, W, n;  // C: channels of label (pred has C + 1); n = B * H * W
  int real;
};

struct GanPixel {
  const float *p, *l;  // channel 0 of this pixel
  double w, mx, sum, lse;
};

// Channel 0 of pred counts as 0 (upstream overwrites it); the log-sum-exp subtracts the pixel's maximum.
__device__ __forceinline__ GanPixel gan_pixel(const GanArgs& s, unsigned i) {
  const unsigned x = i % s.W, r = i / s.W, y = r % s.H, b = r / s.H;
  GanPixel px;
  px.p = s.pred + (b * s.p_bs + y * s.p_rs + x);
  px.l = s.label + (b * s.l_bs + y * s.l_rs + x);
  px.w = s.weight ? (double)s.weight[b * s.w_bs + y * s.w_rs + x] : 1.0;
  float top = 0.0f;
  for (unsigned c = 1; c <= s.C; c++) top = fmaxf(top, px.p[c * s.p_cs]);
  const double mx = (double)top;
  double sum = exp(0.0 - mx);
  for (unsigned c = 1; c <= s.C; c++) sum += exp((double)px.p[c * s.p_cs] - mx);
  px.mx = mx;
  px.sum = sum;
  px.lse = mx + log(sum);
  return px;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_gan_partials(const GanArgs s, double* __restrict__ partials) {
  __shared__ double lds[LOSS_BLOCK / 64];
  const unsigned i = blockIdx.x * (unsigned)GAN_ITEMS + threadIdx.x;
  double per = 0.0;
  if (i < s.n) {
    const GanPixel px = gan_pixel(s, i);
    if (s.real) {  // label channel 0 counts as 0
      for (unsigned c = 1; c < s.C; c++) per += (double)px.l[c * s.l_cs] * (px.lse - (double)px.p[c * s.p_cs]);
    } else {
      per = px.lse - (double)px.p[s.C * s.p_cs];
    }
    if (s.weight) per = per * px.w;
  }
  per = block_sum(per, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = per;
}

// dpred contiguous [B][C + 1][H][W]: k (softmax_c S - lab_c) in the real mode (S the sum of the labels that count,
// lab_0 = lab_C = 0), k (softmax_c - [c = C]) in the fake mode, k = g / count * weight; channel 0 exactly 0.  Evaluated
// in binary64 like the forward, one rounding to float at the store.
__global__ __launch_bounds__(LOSS_BLOCK) void k_gan_backward(const GanArgs s, const float* __restrict__ g, double count,
                                                            float* __restrict__ dpred) {
  const unsigned i = blockIdx.x * (unsigned)LOSS_BLOCK + threadIdx.x;
  if (i >= s.n) return;
  const GanPixel px = gan_pixel(s, i);
  const double k = (double)g[0] / count * px.w;
  const unsigned plane = s.H * s.W, b = i / plane;
  float* d = dpred + ((size_t)b * (s.C + 1) * plane + (i - b * plane));
  double S = 1.0;
  if (s.real) {
    S = 0.0;
    for (unsigned c = 1; c < s.C; c++) S += (double)px.l[c * s.l_cs];
  }
  d[0] = 0.0f;
  for (unsigned c = 1; c <= s.C; c++) {
    const double soft = exp((double)px.p[c * s.p_cs] - px.mx) / px.sum;
    const double target = s.real ? (c < s.C ? (double)px.l[c * s.l_cs] : 0.0) : (c == s.C ? 1.0 : 0.0);
    d[(size_t)c * plane] = (float)(k * (soft * S - target));
  }
}

// ---- K22 ---------------------------------------------------------------------------------------------------------
struct LabelArgs {
  const float *seg, *mask;  // mask: or null
  long long s_bs, s_cs, s_rs, m_bs, m_rs;  // elements; the pixel stride is 1
  unsigned B, C, H, W, h, w, n;  // n = B * h * w
  float* out;                    // contiguous [B][C][h][w]
};

// adaptive_avg_pool2d's window of output index i: [floor(i N / n), ceil((i + 1) N / n))
__device__ __forceinline__ void pool_window(unsigned i, unsigned N, unsigned n, unsigned& lo, unsigned& hi) {
  lo = (unsigned)(((unsigned long long)i * N) / n);
  hi = (unsigned)(((unsigned long long)(i + 1) * N + n - 1) / n);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_label_map(const LabelArgs s) {
  const unsigned i = blockIdx.x * (unsigned)LOSS_BLOCK + threadIdx.x;
  if (i >= s.n) return;
  const unsigned ox = i % s.w, r = i / s.w, oy = r % s.h, b = r / s.h;
  unsigned y0, y1, x0, x1;
  pool_window(oy, s.H, s.h, y0, y1);
  pool_window(ox, s.W, s.w, x0, x1);
  const float* seg = s.seg + b * s.s_bs;
  const float* mask = s.mask ? s.mask + b * s.m_bs : nullptr;
  unsigned best = 0;
  float best_sum = 0.0f;
  for (unsigned c = 0; c < s.C; c++) {
    const float* sc = seg + c * s.s_cs;
    float acc = 0.0f;
    for (unsigned y = y0; y < y1; y++) {
      for (unsigned x = x0; x < x1; x++) {
        float v = sc[y * s.s_rs + x];
        if (mask) v = v * mask[y * s.m_rs + x];
        acc += v;
      }
    }
    if (c == 0 || acc > best_sum) {  // a tie stays with the lower channel
      best = c;
      best_sum = acc;
    }
  }
  const size_t plane = (size_t)s.h * s.w;
  float* o = s.out + ((size_t)b * s.C * plane + (size_t)oy * s.w + ox);
  for (unsigned c = 0; c < s.C; c++) o[c * plane] = c == best ? 1.0f : 0.0f;
}

// ---- host ----------------------------------------------------------------------------------------------------------
// Elements from the first to one past the last of a [B][C][H][W] view with these strides.
int64_t view_extent(int64_t B, int64_t C, int64_t H, int64_t W, int64_t bs, int64_t cs, int64_t rs) {
  return (B - 1) * bs + (C - 1) * cs + (H - 1) * rs + W;
}
bool ranges_overlap(const float* out, int64_t out_n, const float* in, int64_t in_n) {
  return out && in && out < in + in_n && in < out + out_n;
}
// (a double partial sum is two floats)
const float* as_floats(const double* p) { return reinterpret_cast<const float*>(p); }

}  // namespace

extern "C" {

int gcv_image_loss_max_classes(void) { return LOSS_MAX_CLASSES; }

int64_t gcv_image_loss_partials(int64_t n_items, int32_t items_are_pixels) {
  if (n_items <= 0 || n_items >= ((int64_t)1 << 31)) {
    fail(GCV_ERR_INVALID_ARGUMENT, "gcv_image_loss_partials: the item count must be in [1, 2^31)");
    return 0;
  }
  const int64_t per = items_are_pixels ? GAN_ITEMS : L1_ITEMS;
  return (n_items + per - 1) / per;
}

static int l1_args(const char* fn, L1Args& s, const float* a, const int64_t a_strides[3], const float* b,
                   const int64_t b_strides[3], const float* mask, const int64_t mask_strides[2], int32_t batch,
                   int32_t channels, int32_t height, int32_t width) {
  const std::string f(fn);
  if (!a || !b || !a_strides || !b_strides || (mask && !mask_strides)) return fail(GCV_ERR_INVALID_ARGUMENT, f + ": null a / b / strides");
  if (batch <= 0 || channels <= 0 || height <= 0 || width <= 0)
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": batch, channels, height and width must be positive");
  if ((int64_t)batch * channels * height * width >= ((int64_t)1 << 31))
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": more than 2^31 - 1 elements");
  for (int k = 0; k < 3; k++)
    if (a_strides[k] < 0 || b_strides[k] < 0 || (mask && k < 2 && mask_strides[k] < 0))
      return fail(GCV_ERR_INVALID_ARGUMENT, f + ": negative stride");
  if (misaligned(a, 4) || misaligned(b, 4) || misaligned(mask, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, f + ": misaligned a / b / mask");
  s.a = a; s.b = b; s.mask = mask;
  s.a_bs = a_strides[0]; s.a_cs = a_strides[1]; s.a_rs = a_strides[2];
  s.b_bs = b_strides[0]; s.b_cs = b_strides[1]; s.b_rs = b_strides[2];
  s.m_bs = mask ? mask_strides[0] : 0; s.m_rs = mask ? mask_strides[1] : 0;
  s.B = (unsigned)batch; s.C = (unsigned)channels; s.H = (unsigned)height; s.W = (unsigned)width;
  s.n = s.B * s.C * s.H * s.W;
  return 0;
}

// true where `out` (out_n floats) overlaps one of the three inputs of K20
static bool l1_overlaps(const L1Args& s, const float* out, int64_t out_n) {
  return ranges_overlap(out, out_n, s.a, view_extent(s.B, s.C, s.H, s.W, s.a_bs, s.a_cs, s.a_rs)) ||
         ranges_overlap(out, out_n, s.b, view_extent(s.B, s.C, s.H, s.W, s.b_bs, s.b_cs, s.b_rs)) ||
         ranges_overlap(out, out_n, s.mask, view_extent(s.B, 1, s.H, s.W, s.m_bs, 0, s.m_rs));
}

int gcv_mean_abs_forward(const float* a, const int64_t a_strides[3], const float* b, const int64_t b_strides[3], const float* mask,
                   const int64_t mask_strides[2], int32_t batch, int32_t channels, int32_t height, int32_t width,
                   double* partials, int64_t n_partials, float* loss, void* hip_stream) {
  L1Args s;
  if (int rc = l1_args("gcv_mean_abs_forward", s, a, a_strides, b, b_strides, mask, mask_strides, batch, channels, height, width)) return rc;
  if (!partials || !loss) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_forward: null partials / loss");
  const int64_t need = ((int64_t)s.n + L1_ITEMS - 1) / L1_ITEMS;
  if (n_partials < need) return fail(GCV_ERR_BUFFER_TOO_SMALL, "gcv_mean_abs_forward: partials holds fewer than gcv_image_loss_partials(n, 0) doubles");
  if (misaligned(partials, 8) || misaligned(loss, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_forward: misaligned partials / loss");
  if (l1_overlaps(s, as_floats(partials), 2 * need) || l1_overlaps(s, loss, 1) || ranges_overlap(loss, 1, as_floats(partials), 2 * need))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_forward: partials / loss overlap an input or each other");
  hipStream_t st = (hipStream_t)hip_stream;
  k_l1_partials<<<dim3((unsigned)need), dim3(LOSS_BLOCK), 0, st>>>(s, partials);
  HIP_TRY(hipGetLastError(), "l1 partial sums launch");
  k_loss_fold<<<dim3(1), dim3(LOSS_BLOCK), 0, st>>>(partials, (unsigned)need, (double)s.n, loss);
  HIP_TRY(hipGetLastError(), "l1 fold launch");
  return 0;
}

int gcv_mean_abs_backward(const float* a, const int64_t a_strides[3], const float* b, const int64_t b_strides[3], const float* mask,
                    const int64_t mask_strides[2], int32_t batch, int32_t channels, int32_t height, int32_t width,
                    const float* grad_loss, float* da, float* db, void* hip_stream) {
  L1Args s;
  if (int rc = l1_args("gcv_mean_abs_backward", s, a, a_strides, b, b_strides, mask, mask_strides, batch, channels, height, width)) return rc;
  if (!grad_loss) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_backward: null grad_loss");
  if (!da && !db) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_backward: null da and db (nothing to write)");
  if (misaligned(grad_loss, 4) || misaligned(da, 4) || misaligned(db, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_backward: misaligned grad_loss / da / db");
  if (l1_overlaps(s, da, s.n) || l1_overlaps(s, db, s.n) || ranges_overlap(da, s.n, db, s.n) || ranges_overlap(da, s.n, grad_loss, 1) ||
      ranges_overlap(db, s.n, grad_loss, 1))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_mean_abs_backward: da / db overlap an input or each other");
  k_l1_backward<<<dim3((s.n + LOSS_BLOCK - 1) / LOSS_BLOCK), dim3(LOSS_BLOCK), 0, (hipStream_t)hip_stream>>>(s, grad_loss, (double)s.n, da, db);
  HIP_TRY(hipGetLastError(), "l1 backward launch");
  return 0;
}

static int gan_args(const char* fn, GanArgs& s, const float* pred, const int64_t pred_strides[3], const float* label,
                    const int64_t label_strides[3], const float* weight, const int64_t weight_strides[2], int32_t batch,
                    int32_t classes, int32_t height, int32_t width, int32_t real) {
  const std::string f(fn);
  if (!pred || !label || !pred_strides || !label_strides || (weight && !weight_strides))
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": null pred / label / strides");
  if (batch <= 0 || classes <= 0 || height <= 0 || width <= 0)
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": batch, classes, height and width must be positive");
  if (classes > LOSS_MAX_CLASSES) return fail(GCV_ERR_INVALID_ARGUMENT, f + ": more than gcv_image_loss_max_classes() classes");
  if ((int64_t)batch * (classes + 1) * height * width >= ((int64_t)1 << 31))
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": more than 2^31 - 1 elements");
  for (int k = 0; k < 3; k++)
    if (pred_strides[k] < 0 || label_strides[k] < 0 || (weight && k < 2 && weight_strides[k] < 0))
      return fail(GCV_ERR_INVALID_ARGUMENT, f + ": negative stride");
  if (misaligned(pred, 4) || misaligned(label, 4) || misaligned(weight, 4))
    return fail(GCV_ERR_INVALID_ARGUMENT, f + ": misaligned pred / label / weight");
  s.pred = pred; s.label = label; s.weight = weight;
  s.p_bs = pred_strides[0]; s.p_cs = pred_strides[1]; s.p_rs = pred_strides[2];
  s.l_bs = label_strides[0]; s.l_cs = label_strides[1]; s.l_rs = label_strides[2];
  s.w_bs = weight ? weight_strides[0] : 0; s.w_rs = weight ? weight_strides[1] : 0;
  s.B = (unsigned)batch; s.C = (unsigned)classes; s.H = (unsigned)height; s.W = (unsigned)width;
  s.n = s.B * s.H * s.W;
  s.real = real != 0;
  return 0;
}

static bool gan_overlaps(const GanArgs& s, const float* out, int64_t out_n) {
  return ranges_overlap(out, out_n, s.pred, view_extent(s.B, s.C + 1, s.H, s.W, s.p_bs, s.p_cs, s.p_rs)) ||
         ranges_overlap(out, out_n, s.label, view_extent(s.B, s.C, s.H, s.W, s.l_bs, s.l_cs, s.l_rs)) ||
         ranges_overlap(out, out_n, s.weight, view_extent(s.B, 1, s.H, s.W, s.w_bs, 0, s.w_rs));
}

int gcv_gan_loss_forward(const float* pred, const int64_t pred_strides[3], const float* label, const int64_t label_strides[3],
                         const float* weight, const int64_t weight_strides[2], int32_t batch, int32_t classes, int32_t height,
                         int32_t width, int32_t real, double* partials, int64_t n_partials, float* loss, void* hip_stream) {
  GanArgs s;
  if (int rc = gan_args("gcv_gan_loss_forward", s, pred, pred_strides, label, label_strides, weight, weight_strides, batch, classes,
                        height, width, real)) return rc;
  if (!partials || !loss) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_forward: null partials / loss");
  const int64_t need = ((int64_t)s.n + GAN_ITEMS - 1) / GAN_ITEMS;
  if (n_partials < need) return fail(GCV_ERR_BUFFER_TOO_SMALL, "gcv_gan_loss_forward: partials holds fewer than gcv_image_loss_partials(n, 1) doubles");
  if (misaligned(partials, 8) || misaligned(loss, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_forward: misaligned partials / loss");
  if (gan_overlaps(s, as_floats(partials), 2 * need) || gan_overlaps(s, loss, 1) || ranges_overlap(loss, 1, as_floats(partials), 2 * need))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_forward: partials / loss overlap an input or each other");
  hipStream_t st = (hipStream_t)hip_stream;
  k_gan_partials<<<dim3((unsigned)need), dim3(LOSS_BLOCK), 0, st>>>(s, partials);
  HIP_TRY(hipGetLastError(), "gan loss partial sums launch");
  k_loss_fold<<<dim3(1), dim3(LOSS_BLOCK), 0, st>>>(partials, (unsigned)need, (double)s.n, loss);
  HIP_TRY(hipGetLastError(), "gan loss fold launch");
  return 0;
}

int gcv_gan_loss_backward(const float* pred, const int64_t pred_strides[3], const float* label, const int64_t label_strides[3],
                          const float* weight, const int64_t weight_strides[2], int32_t batch, int32_t classes, int32_t height,
                          int32_t width, int32_t real, const float* grad_loss, float* dpred, void* hip_stream) {
  GanArgs s;
  if (int rc = gan_args("gcv_gan_loss_backward", s, pred, pred_strides, label, label_strides, weight, weight_strides, batch, classes,
                        height, width, real)) return rc;
  if (!grad_loss || !dpred) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_backward: null grad_loss / dpred");
  if (misaligned(grad_loss, 4) || misaligned(dpred, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_backward: misaligned grad_loss / dpred");
  const int64_t out_n = (int64_t)s.n * (s.C + 1);
  if (gan_overlaps(s, dpred, out_n) || ranges_overlap(dpred, out_n, grad_loss, 1))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_gan_loss_backward: dpred overlaps an input");
  k_gan_backward<<<dim3((s.n + LOSS_BLOCK - 1) / LOSS_BLOCK), dim3(LOSS_BLOCK), 0, (hipStream_t)hip_stream>>>(s, grad_loss, (double)s.n, dpred);
  HIP_TRY(hipGetLastError(), "gan loss backward launch");
  return 0;
}

int gcv_label_map(const float* seg, const int64_t seg_strides[3], const float* mask, const int64_t mask_strides[2], int32_t batch,
                  int32_t classes, int32_t height, int32_t width, int32_t out_height, int32_t out_width, float* out,
                  void* hip_stream) {
  if (!seg || !seg_strides || !out || (mask && !mask_strides)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: null seg / strides / out");
  if (batch <= 0 || classes <= 0 || height <= 0 || width <= 0 || out_height <= 0 || out_width <= 0)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: batch, classes and the four sizes must be positive");
  if (classes > LOSS_MAX_CLASSES) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: more than gcv_image_loss_max_classes() classes");
  if (out_height > height || out_width > width)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: the target size exceeds the source size");
  if ((int64_t)batch * classes * height * width >= ((int64_t)1 << 31))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: more than 2^31 - 1 elements");
  for (int k = 0; k < 3; k++)
    if (seg_strides[k] < 0 || (mask && k < 2 && mask_strides[k] < 0)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: negative stride");
  if (misaligned(seg, 4) || misaligned(mask, 4) || misaligned(out, 4)) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: misaligned seg / mask / out");
  LabelArgs s;
  s.seg = seg; s.mask = mask;
  s.s_bs = seg_strides[0]; s.s_cs = seg_strides[1]; s.s_rs = seg_strides[2];
  s.m_bs = mask ? mask_strides[0] : 0; s.m_rs = mask ? mask_strides[1] : 0;
  s.B = (unsigned)batch; s.C = (unsigned)classes; s.H = (unsigned)height; s.W = (unsigned)width;
  s.h = (unsigned)out_height; s.w = (unsigned)out_width; s.n = s.B * s.h * s.w;
  s.out = out;
  const int64_t out_n = (int64_t)s.n * s.C;
  if (ranges_overlap(out, out_n, seg, view_extent(s.B, s.C, s.H, s.W, s.s_bs, s.s_cs, s.s_rs)) ||
      ranges_overlap(out, out_n, mask, view_extent(s.B, 1, s.H, s.W, s.m_bs, 0, s.m_rs)))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_label_map: out overlaps an input");
  k_label_map<<<dim3((s.n + LOSS_BLOCK - 1) / LOSS_BLOCK), dim3(LOSS_BLOCK), 0, (hipStream_t)hip_stream>>>(s);
  HIP_TRY(hipGetLastError(), "label map launch");
  return 0;
}

}  // extern "C"
