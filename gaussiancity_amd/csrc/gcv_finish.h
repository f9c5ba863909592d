// gcv_finish.h -- K19 (frame finish: road-mask blur, composite and the video bytes in one launch) of libgcv_hip.so;
// included by gcv_points.hip, whose helpers (fail, HIP_TRY, misaligned) it uses.
// Reference behaviour: scripts/inference.py:255,264-272 (GaussianBlur on the float image, blended back through the road
// mask of ins_map) followed by :665-667 (tensor_to_image * 255 -> uint8, optionally BGR).
//
// One thread per pixel, a block of 64 x 4 pixels, the three channels in the thread.  A thread reads its mask value; a
// pixel that shows no road copies its three floats, a road pixel evaluates the (2r+1)^2 stencil per channel with plain
// global loads of its neighbours (reflect indexing, no halo tile): the frame is a few MB and stays in the caches, the
// neighbours of a wave's 64 consecutive pixels are the same cache lines three times over, and only lanes on a road take
// the loads at all.  No LDS, no barrier, no atomics, no workspace; a pixel's value is a function of its own coordinates
// alone, so it cannot depend on the tiling.  The sum is float32 in row-major tap order starting from the first product,
// one rounding per product and per addition (the library is built with -ffp-contract=off).
#pragma once

namespace {

constexpr int FF_RADIUS_MAX = 3;
constexpr int FF_BLOCK_X = 64, FF_BLOCK_Y = 4;

struct FinishArgs {
  const float* img;
  long long batch_stride, channel_stride, row_stride;  // elements; the pixel stride is 1
  int H, W;
  const int16_t* map;
  long long map_batch_stride;  // 0: one map for every image
  int road_id, flip_mask_x, bgr;
  float* out_f32;    // or null; [B][3][H][W]
  uint8_t* out_u8;   // or null; [B][H][W][3]
  float w[(2 * FF_RADIUS_MAX + 1) * (2 * FF_RADIUS_MAX + 1)];
};

// InferenceLoop.to_uint8_hwc per value, the expression of the blend kernel's out_u8 store: one rounding per step,
// truncation, a NaN becomes 0.
__device__ __forceinline__ uint8_t ff_video_byte(float c) {
  float t = c < -1.0f ? -1.0f : (c > 1.0f ? 1.0f : c);
  t = t / 2.0f;
  t = t + 0.5f;
  t = t * 255.0f;
  return (uint8_t)(t == t ? (int)t : 0);
}

// torch's "reflect" padding without repeating the edge: -1 -> 1, n -> n - 2.  One reflection is enough for n > radius.
__device__ __forceinline__ int ff_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

template <int R>
__global__ __launch_bounds__(FF_BLOCK_X * FF_BLOCK_Y) void k_frame_finish(const FinishArgs a) {
  constexpr int K = 2 * R + 1;
  const int x = (int)blockIdx.x * FF_BLOCK_X + (int)threadIdx.x;
  const int y = (int)blockIdx.y * FF_BLOCK_Y + (int)threadIdx.y;
  const long long b = blockIdx.z;
  if (x >= a.W || y >= a.H) return;
  const int mx = a.flip_mask_x ? a.W - 1 - x : x;
  const bool road = (int)a.map[b * a.map_batch_stride + (long long)y * a.W + mx] == a.road_id;
  const float* img = a.img + b * a.batch_stride;
  float v[3];
  if (!road) {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = img[c * a.channel_stride + y * a.row_stride + x];
  } else {
    long long row[K];
    int col[K];
#pragma unroll
    for (int d = 0; d < K; d++) {
      row[d] = ff_reflect(y + d - R, a.H) * a.row_stride;
      col[d] = ff_reflect(x + d - R, a.W);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float* p = img + c * a.channel_stride;
      float acc = 0.0f;
#pragma unroll
      for (int dy = 0; dy < K; dy++) {
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
          const float t = a.w[dy * K + dx] * p[row[dy] + col[dx]];
          acc = (dy == 0 && dx == 0) ? t : acc + t;
        }
      }
      v[c] = acc;
    }
  }
  const long long plane = (long long)a.H * a.W, pix = (long long)y * a.W + x;
  if (a.out_f32) {
    float* o = a.out_f32 + b * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c * plane] = v[c];
  }
  if (a.out_u8) {
    uint8_t* o = a.out_u8 + (b * plane + pix) * 3;
    o[0] = ff_video_byte(a.bgr ? v[2] : v[0]);
    o[1] = ff_video_byte(v[1]);
    o[2] = ff_video_byte(a.bgr ? v[0] : v[2]);
  }
}

}  // namespace

extern "C" {

int gcv_frame_finish_radius_max(void) { return FF_RADIUS_MAX; }

int gcv_frame_finish(const float* img, int64_t batch_stride, int64_t channel_stride, int64_t row_stride, int32_t batch,
                     int32_t height, int32_t width, const int16_t* ins_map, int64_t map_batch_stride, int32_t road_id,
                     int32_t flip_mask_x, int32_t radius, const float* weights_host, float* out_f32, uint8_t* out_u8,
                     int32_t bgr, void* hip_stream) {
  if (!img || !ins_map || !weights_host) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: null img / ins_map / weights_host");
  if (!out_f32 && !out_u8) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: null out_f32 and out_u8 (nothing to write)");
  if (radius < 1 || radius > FF_RADIUS_MAX) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: radius must be 1, 2 or 3");
  if (batch <= 0 || height <= 0 || width <= 0) return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: batch, height and width must be positive");
  if (height <= radius || width <= radius)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: reflect padding needs height and width above the radius");
  if (batch_stride < 0 || channel_stride < 0 || row_stride < 0 || map_batch_stride < 0)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: negative stride");
  if (batch > 65535 || (height + FF_BLOCK_Y - 1) / FF_BLOCK_Y > 65535)
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: batch above 65535 or height above 262140");
  if (misaligned(img, 4) || misaligned(ins_map, 2) || misaligned(out_f32, 4))
    return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: misaligned img / ins_map / out_f32");
  if (out_f32) {  // the stencil reads neighbours other threads may already have overwritten: not in place
    const int64_t extent = (batch - 1) * batch_stride + 2 * channel_stride + (height - 1) * row_stride + width;
    const int64_t out_n = (int64_t)batch * 3 * height * width;
    if (out_f32 < img + extent && img < out_f32 + out_n)
      return fail(GCV_ERR_INVALID_ARGUMENT, "gcv_frame_finish: out_f32 overlaps the image (the stencil cannot run in place)");
  }
  FinishArgs a;
  a.img = img; a.batch_stride = batch_stride; a.channel_stride = channel_stride; a.row_stride = row_stride;
  a.H = height; a.W = width; a.map = ins_map; a.map_batch_stride = map_batch_stride;
  a.road_id = road_id; a.flip_mask_x = flip_mask_x != 0; a.bgr = bgr != 0; a.out_f32 = out_f32; a.out_u8 = out_u8;
  const int taps = (2 * radius + 1) * (2 * radius + 1);
  for (int k = 0; k < (int)(sizeof(a.w) / sizeof(a.w[0])); k++) a.w[k] = k < taps ? weights_host[k] : 0.0f;
  const dim3 grid((unsigned)((width + FF_BLOCK_X - 1) / FF_BLOCK_X), (unsigned)((height + FF_BLOCK_Y - 1) / FF_BLOCK_Y), (unsigned)batch);
  const dim3 block(FF_BLOCK_X, FF_BLOCK_Y);
  hipStream_t s = (hipStream_t)hip_stream;
  switch (radius) {
    case 1: k_frame_finish<1><<<grid, block, 0, s>>>(a); break;
    case 2: k_frame_finish<2><<<grid, block, 0, s>>>(a); break;
    default: k_frame_finish<3><<<grid, block, 0, s>>>(a); break;
  }
  HIP_TRY(hipGetLastError(), "frame finish launch");
  return 0;
}

}  // extern "C"
