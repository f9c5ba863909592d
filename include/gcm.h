/*
 * gcm.h -- C ABI of the MI355X-native grouped modulated MLP of the generator's attribute head (libgcm_hip.so).
 *
 * GaussianCity's GaussianAttrMLP (models/generator.py) runs its ModLinear layers once per building instance: a
 * boolean-mask gather, a modulated copy of the weight, three small products and a scatter for every instance.  With
 * output_mode a ModLinear is y = (x o alpha(z)) W^T + beta(z): only the vectors alpha and beta depend on the instance,
 * so every instance goes through ONE product per layer with a per-row lookup of alpha[group] and beta[group].  This
 * library holds those kernels; gaussiancity_amd/modlinear.py is the autograd layer and gaussiancity_amd/attr_head.py
 * rebinds the method.  DESIGN.md section 17.
 *
 * Conventions as gca.h: raw DEVICE pointers, a HIP stream appended, 0 or a negative gcm_status returned,
 * gcm_last_error() has the text.  Arguments are checked before anything is queued on the device, no call allocates
 * and no call waits for the device.  Everything is float32.
 *
 *   N, I, O     rows, input and output features.  N >= 0; I and O positive multiples of 4 (at most 65536).
 *   G           groups, 1 .. 2^20.  A plain linear layer is G = 1 with group == NULL.
 *   x, y, dy, dx   row-strided: element (r, c) at p[r * stride + c]; strides are in ELEMENTS, positive multiples of 4
 *               and at least the row's width.  w is [O][I] with row stride w_stride under the same rule.
 *   alpha [G][I], beta [G][O], bias [O]   contiguous; each may be NULL (alpha: ones, beta and bias: zeros).
 *   group       int32 [N] or NULL (every row in group 0).  A value outside 0 .. G-1 is "no group" (-1): the row's y
 *               and dx are exact zeros and it contributes to no gradient.
 *   slope       LeakyReLU's negative slope, finite and > 0; 1 means no activation.
 *   Every float pointer is 16-byte aligned.
 *
 * gcm_modlinear_forward:   y[r] = act((x[r] o alpha[g]) W^T + beta[g] + bias), g = group[r].
 * gcm_modlinear_backward:  dpre = dy o (y > 0 ? 1 : slope) from the STORED y (torch's leaky_relu rule at 0),
 *     dxs = dpre W, dx = dxs o alpha[g];  dw [O][I] = dpre^T (x o alpha[g]);  dalpha[g] = sum over the rows r of g of
 *     dxs[r] o x[r];  dbeta[g] = sum over the rows of g of dpre[r];  dbias = sum over g of dbeta[g].
 *     dw, dalpha [G][I], dbeta [G][O] and dbias [O] are contiguous; each output is written whole (an empty group's
 *     rows are exact zeros), a NULL output is skipped.  workspace is gcm_modlinear_backward_workspace_bytes(N, I, O, G)
 *     bytes, 256-byte aligned; what it held before does not matter.
 *
 * Rounding: x o alpha is one fp32 product; every product of two matrices runs on the exact f32-input matrix
 * instruction (v_mfma_f32_16x16x4_f32), one fp32 fmaf chain from 0 in the order of the summed index; beta, then bias
 * are added in fp32 after the chain.  No float atomics anywhere: dw is the sum of row slices in slice order, the
 * per-group sums run over the group's rows in ascending row order (a stable counting sort by group), in slices
 * folded in slice order, dbias adds the groups in ascending order.  Every output is bit-identical run to run.
 *
 * gcm_groups_from_masks: masks is a DEVICE array of G pointers to N-byte boolean masks; group[r] is the largest g
 *     with masks[g][r] != 0 (a later mask wins where masks overlap), -1 where none is set.  One launch whatever G is.
 *
 * gcm_head_out (inference): out[r][c] = T(f[r] . w_out[c] + b[c]), c < C, C = 1 or 3, out contiguous [N][C], w_out
 *     contiguous [C][I], b [C] or NULL.  T by gcm_kind:
 *       GCM_XYZ, GCM_RGB   (sigmoid(v) - 1/2) * factor
 *       GCM_SCALE          1 + clamp(v, -1, 1) * factor
 *       GCM_OPACITY        sigmoid(v) * factor + (1 - factor)
 *     The dot product is fp32 (a fixed tree over I), T is evaluated in double and rounded once.  Rows with a
 *     negative group are exact zeros (group NULL: every row has one).
 */
#ifndef GCM_H
#define GCM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCM_ABI_VERSION 1

enum gcm_status { GCM_OK = 0, GCM_ERR_INVALID_ARGUMENT = -1, GCM_ERR_HIP = -2 };

enum gcm_kind { GCM_XYZ = 0, GCM_RGB = 1, GCM_SCALE = 2, GCM_OPACITY = 3 };

int gcm_abi_version(void);
const char* gcm_last_error(void);

int gcm_groups_from_masks(const void* masks, int64_t G, int64_t N, int32_t* group, void* hip_stream);

int gcm_modlinear_forward(const float* x, int64_t x_stride, const float* w, int64_t w_stride, const float* alpha,
                          const float* beta, const float* bias, const int32_t* group, int64_t N, int32_t I, int32_t O,
                          int32_t G, float slope, float* y, int64_t y_stride, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_modlinear_backward_workspace_bytes(int64_t N, int32_t I, int32_t O, int32_t G);

int gcm_modlinear_backward(const float* x, int64_t x_stride, const float* y, int64_t y_stride, const float* dy,
                           int64_t dy_stride, const float* w, int64_t w_stride, const float* alpha,
                           const int32_t* group, int64_t N, int32_t I, int32_t O, int32_t G, float slope, float* dx,
                           int64_t dx_stride, float* dw, float* dalpha, float* dbeta, float* dbias, void* workspace,
                           size_t workspace_bytes, void* hip_stream);

int gcm_head_out(const float* f, int64_t f_stride, const float* w_out, const float* b, const int32_t* group, int64_t N,
                 int32_t I, int32_t C, int kind, float factor, float* out, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
