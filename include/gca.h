/*
 * gca.h -- C ABI of the MI355X-native variable-length attention of the point backbone (libgca_hip.so).
 *
 * The PTv3 backbone of GaussianCity's generators (models/pt_v3.py) calls flash_attn's
 * flash_attn_varlen_qkvpacked_func once per block.  This library holds that operator's kernels;
 * gaussiancity_amd/attention.py is the autograd layer and flash_attn/ at the repository root is the drop-in
 * module.  DESIGN.md section 16.
 *
 * Conventions as gcs.h: raw DEVICE pointers, a HIP stream appended, 0 or a negative gca_status returned,
 * gca_last_error() has the text.  Arguments are checked before anything is queued on the device, and no call waits
 * for the device.
 *
 *   qkv         binary16, element (row, slot, head, c) at qkv[row * row_stride + slot * slot_stride +
 *               head * head_stride + c]; slot 0 / 1 / 2 is the query / key / value, c < head_dim has unit stride.
 *               Strides are in ELEMENTS, positive multiples of 8; the pointer is 16-byte aligned.
 *   cu_seqlens  int32 [nseg + 1]; segment s is rows cu_seqlens[s] .. cu_seqlens[s + 1] - 1.  Entries are clamped
 *               to [0, total] on the device, a negative length counts as 0, a length above max_seqlen is cut to
 *               its first max_seqlen rows.  The vector is never read on the host.
 *   out         binary16 [total][heads][head_dim], contiguous; per segment and head
 *               softmax(softmax_scale * Q K^T) V.  Rows that no segment covers are zeros.
 *   lse         float [heads][total]: log(sum_j exp(softmax_scale * q_i . k_j)) of the row (0 where uncovered).
 *   head_dim    16, 32 or 64.
 *
 * gca_varlen_backward: dout is binary16, element (row, head, c) at dout[row * dout_row_stride +
 * head * dout_head_stride + c] (same stride rules); dqkv is binary16 [total][3][heads][head_dim], contiguous, and
 * is WRITTEN (zeros where no segment covers the row); workspace is gca_backward_workspace_bytes(total, heads) bytes.
 * No float atomics anywhere: out, lse and dqkv are bit-identical run to run.
 *
 * Rounding: inputs are read as binary16, every product accumulates in fp32 on the matrix cores, the softmax
 * maximum, row sum and log-sum-exp are fp32, the probabilities and dS are rounded to binary16 as matrix-core
 * operands, out and dqkv are rounded to binary16 once, on store.
 *
 * The `_t` entry points take the element type of qkv, out, dout and dqkv first (gca_dtype; gca_dtypes() has a bit
 * 1 << dtype for every one the library runs).  GCA_F16 is the above, launch for launch and bit for bit.  GCA_F32:
 * the same arguments and layouts in binary32, strides positive multiples of 4 elements, pointers 16-byte aligned;
 * lse, the workspace and every guarantee above are unchanged.
 *
 * Rounding, float32: inputs are read as binary32 and every product runs on the exact f32-input matrix instruction,
 * a fp32 fmaf chain in the order of the summed index, one rounding per term.  Scores, the softmax maximum, row sum,
 * log-sum-exp, the probabilities, dS and D = rowsum(dout o out) -- from the stored out -- are fp32; nothing is
 * rounded to binary16 anywhere; out and dqkv are stored as binary32.  Exponents are in natural units: the score is
 * the fp32 product (q . k) * scale in the forward and in the backward alike, the exponential is the hardware's exp2
 * of the exponent times log2(e) (about 1 ulp), and lse is maximum + log(row sum) rounded to binary32 ONCE (the
 * per-row logarithm runs in double).  The backward recomputes P = exp(score - lse) with the rounding errors of the
 * difference and of its product with log2(e) computed and applied, so that the size of lse -- about log(keys),
 * whatever the scores -- costs a probability nothing beyond that one rounding per row; where one key holds all the
 * weight of a row, P is exactly 1 and 0.
 */
#ifndef GCA_H
#define GCA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCA_ABI_VERSION 1

enum gca_status { GCA_OK = 0, GCA_ERR_INVALID_ARGUMENT = -1, GCA_ERR_HIP = -2 };

enum gca_dtype { GCA_F16 = 0, GCA_F32 = 1 };

int gca_abi_version(void);
const char* gca_last_error(void);
int gca_dtypes(void); /* bit 1 << dtype for every gca_dtype the `_t` entry points run: 3 */

/* size queries; 0 with a message in gca_last_error() when an argument is out of range (a valid empty problem,
 * total == 0, also gives 0 and clears the message) */
size_t gca_lse_bytes(int64_t total, int32_t heads);
size_t gca_backward_workspace_bytes(int64_t total, int32_t heads);

int gca_varlen_forward(const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                       const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim,
                       int64_t max_seqlen, float softmax_scale, void* out, float* lse, void* hip_stream);

int gca_varlen_backward(const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                        const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride,
                        const float* lse, const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads,
                        int32_t head_dim, int64_t max_seqlen, float softmax_scale, void* dqkv, void* workspace,
                        size_t workspace_bytes, void* hip_stream);

/* the two calls above for the element type `dtype`; an unknown dtype is GCA_ERR_INVALID_ARGUMENT */
int gca_varlen_forward_t(int dtype, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                         const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads, int32_t head_dim,
                         int64_t max_seqlen, float softmax_scale, void* out, float* lse, void* hip_stream);

int gca_varlen_backward_t(int dtype, const void* qkv, int64_t row_stride, int64_t slot_stride, int64_t head_stride,
                          const void* out, const void* dout, int64_t dout_row_stride, int64_t dout_head_stride,
                          const float* lse, const int32_t* cu_seqlens, int64_t nseg, int64_t total, int32_t heads,
                          int32_t head_dim, int64_t max_seqlen, float softmax_scale, void* dqkv, void* workspace,
                          size_t workspace_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
