/*
 * gcs.h -- C ABI of the MI355X-native sparse operators of the point backbone (libgcs_hip.so).
 *
 * The PTv3 backbone of GaussianCity's generators (models/pt_v3.py) needs three things from two CUDA-only
 * packages: spconv's submanifold convolution SubMConv3d (with its SparseConvTensor container) and
 * torch_scatter's segment_csr.  This library holds their kernels; gaussiancity_amd/sparse.py is the autograd
 * layer and spconv/, torch_scatter/ at the repository root are the drop-in modules.
 *
 * Conventions as gce.h: raw DEVICE pointers, a HIP stream appended, 0 or a negative gcs_status returned,
 * gcs_last_error() has the text.  Arguments are checked before anything is queued on the device.
 *
 * Submanifold convolution
 *   indices   int32 [N][4]  (b, d0, d1, d2); a row is valid when 0 <= b < batch_size and 0 <= d < spatial_shape.
 *   ksize     three odd kernel sizes, K = ksize[0] * ksize[1] * ksize[2] taps, tap k = (a * ksize[1] + b) * ksize[2] + c.
 *   dilation  three positive dilations.  Tap k of row i is the row at (b_i, p_i + (tap - ksize / 2) * dilation).
 *   Several rows may share one voxel: the voxel's representative is its LOWEST row index, and only
 *   representatives are ever neighbours.  Rows of one voxel therefore get identical outputs.
 *   weight    float [Cout][K][Cin] (spconv 2.x KRSC), bias float [Cout] or NULL.
 *   features  float [N][Cin] row-major, output float [N][Cout].
 *
 * The rulebook is one device buffer of gcs_subm_rulebook_bytes(N, K) bytes that the caller keeps for as long as
 * convolutions reuse it; gcs_subm_rulebook fills it from the indices, using gcs_subm_rulebook_scratch_bytes(N)
 * bytes of scratch that are free again when the stream reaches the end of the call.  With host_info != NULL the
 * call waits once for the stream and writes host_info[0] = number of invalid rows (they have no neighbours and
 * are nobody's neighbour), host_info[1] = 1 if any voxel holds several rows, host_info[2 + k] = rows that have
 * tap k.  gcs_subm_forward / gcs_subm_backward never wait.
 *
 * gcs_subm_backward: dx [N][Cin], dw [Cout][K][Cin], db [Cout] are WRITTEN (not accumulated); any may be NULL.
 * `dups` is host_info[1] of the rulebook (it selects the fold of dy onto the representatives and the
 * gcs_subm_backward_workspace_bytes size).  No float atomics: results are bit-identical run to run.
 *
 * segment_csr (torch_scatter semantics, reduction along dim 0)
 *   src float [M][F], indptr int64 [S + 1] (non-decreasing; entries are clamped to [0, M]), out float [S][F].
 *   reduce GCS_SUM / GCS_MEAN / GCS_MIN / GCS_MAX; an empty segment gives 0.  For min and max `arg` int64 [S][F]
 *   receives the FIRST row that attains the value (-1 for an empty segment), and the backward pass routes the
 *   gradient to it; for sum and mean `arg` is unused.  The backward pass writes all of dsrc [M][F].
 */
#ifndef GCS_H
#define GCS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCS_ABI_VERSION 4
#define GCS_HOST_INFO_HEADER 2 /* host_info words before the per-tap pair counts */

enum gcs_status { GCS_OK = 0, GCS_ERR_INVALID_ARGUMENT = -1, GCS_ERR_HIP = -2 };
enum gcs_reduce { GCS_SUM = 0, GCS_MEAN = 1, GCS_MIN = 2, GCS_MAX = 3 };
/* workgroup tiles (rows x columns) of the convolution kernels, as gcs_subm_plan reports them */
enum gcs_tile { GCS_TILE_32X32 = 0, GCS_TILE_64X64 = 1, GCS_TILE_128X32 = 2 };
/* what runs the convolution's three products, the forward, dX and dW (ABI v3; dW since v4): the VALU kernels, or the
 * same products on the f32 matrix cores */
enum gcs_engine { GCS_ENGINE_VALU = 0, GCS_ENGINE_MFMA = 1 };
/* bits of gcs_engine_products (ABI v4) */
#define GCS_PRODUCT_FORWARD 1
#define GCS_PRODUCT_DX 2
#define GCS_PRODUCT_DW 4

int gcs_abi_version(void);
const char* gcs_last_error(void);

/* workspace queries; 0 means the arguments are out of range (gcs_last_error says why) */
size_t gcs_subm_rulebook_bytes(int64_t n, int32_t kvol);
size_t gcs_subm_rulebook_scratch_bytes(int64_t n);
size_t gcs_subm_backward_workspace_bytes(int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups);

/* Host only, no device work: the kernel variants that gcs_subm_forward / gcs_subm_backward launch for this shape, the
 * one choice they dispatch from.  plan[0] = gcs_tile of the forward (n x cout), plan[1] = gcs_tile of dX (n x cin),
 * plan[2] = gcs_tile of dW, plan[3] = slices of the dW sum, plan[4] = slices of the dB sum.  Tests ask it to make
 * sure that a shape still reaches the variant it was chosen for. */
int gcs_subm_plan(int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t plan[5]);

int gcs_subm_rulebook(const int32_t* indices, int64_t n, int32_t batch_size, const int32_t* spatial_shape,
                      const int32_t* ksize, const int32_t* dilation, void* rulebook, size_t rulebook_bytes,
                      void* scratch, size_t scratch_bytes, int32_t* host_info, void* hip_stream);

int gcs_subm_forward(const void* rulebook, int64_t n, int32_t kvol, const float* features, int32_t cin,
                     const float* weight, const float* bias, int32_t cout, float* out, void* hip_stream);

int gcs_subm_backward(const void* rulebook, int64_t n, int32_t kvol, int32_t dups, const float* features,
                      int32_t cin, const float* weight, int32_t cout, const float* dout, float* dx, float* dw,
                      float* db, void* workspace, size_t workspace_bytes, void* hip_stream);

/* Engines (ABI v3; v4 moved dW to the engine and added gcs_engine_products).  The entry points above are
 * GCS_ENGINE_VALU; the `_engine` calls take the engine as their first argument and are, with GCS_ENGINE_VALU, the
 * calls above: the same launches, the same backward workspace.  With GCS_ENGINE_MFMA the forward and dX run on v_mfma_f32_16x16x4_f32 under the same tiles, with the same summation
 * order per output element (taps in loop order, channels ascending, the bias last): where the plan has one tap slice
 * the values are those of the VALU engine.  A tile grid below 256 workgroups is cut over the taps into S slices whose
 * partial tiles [S][N][columns] go to the workspace and are summed in slice order; the workspace's previous contents
 * never matter.  dW runs on the same instruction under the VALU plan's tile and slice count (plan[2], plan[3]): every
 * element of a slice's partial is one chain from 0 over the slice's pairs in list order under both engines, so dW is
 * the VALU engine's dW bit for bit at every shape, and its share of the workspace is the same.  The sum of the dW
 * slices, dB, the fold of dY, the rulebook and segment_csr are the same kernels under both engines.
 *
 * gcs_engine_products: host only; the products that `engine` runs on the matrix cores, a set of GCS_PRODUCT_* bits:
 * 0 for GCS_ENGINE_VALU, 7 for GCS_ENGINE_MFMA; -1 (GCS_ERR_INVALID_ARGUMENT) for an unknown engine.
 *
 * gcs_subm_engine_plan: plan[0..4] as gcs_subm_plan, plan[5] = tap slices of the forward, plan[6] = tap slices of dX
 * (1, 1 for GCS_ENGINE_VALU).  gcs_subm_engine_workspace_bytes returns a status, so that 0 bytes is a valid answer (a
 * forward with one slice needs none and accepts NULL).  An unknown engine, and a workspace that is missing or too small
 * when the plan needs one, are GCS_ERR_INVALID_ARGUMENT before anything is queued. */
int gcs_engine_products(int32_t engine);
int gcs_subm_engine_plan(int32_t engine, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t plan[7]);
int gcs_subm_engine_workspace_bytes(int32_t engine, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups,
                                    size_t* forward_bytes, size_t* backward_bytes);
int gcs_subm_forward_engine(int32_t engine, const void* rulebook, int64_t n, int32_t kvol, const float* features,
                            int32_t cin, const float* weight, const float* bias, int32_t cout, float* out,
                            void* workspace, size_t workspace_bytes, void* hip_stream);
int gcs_subm_backward_engine(int32_t engine, const void* rulebook, int64_t n, int32_t kvol, int32_t dups,
                             const float* features, int32_t cin, const float* weight, int32_t cout, const float* dout,
                             float* dx, float* dw, float* db, void* workspace, size_t workspace_bytes, void* hip_stream);

int gcs_segment_csr_forward(const float* src, int64_t m, int64_t f, const int64_t* indptr, int64_t s, int32_t reduce,
                            float* out, int64_t* arg, void* hip_stream);
int gcs_segment_csr_backward(const float* dout, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                             int32_t reduce, const int64_t* arg, float* dsrc, void* hip_stream);


/* Typed entry points: binary16.  GCS_ABI_VERSION stays 4 -- the additions below change no existing symbol, signature or
 * value, so a binding written for v4 keeps working; gcs_dtypes() is how a binding learns whether the library has them.
 * The convention is gce.h's `_t(dtype, ...)`: every typed tensor (features, weight, bias, out, dout, dx, dw, db, src,
 * dsrc) is void* and holds `dtype`; layouts and NULL rules are those of the float entry points; `arg`, `indptr` and the
 * rulebook do not depend on the dtype, and ONE rulebook serves both.
 *
 * GCS_F32: exactly the default entry points above (gcs_subm_forward, gcs_subm_backward with the workspace of
 * gcs_subm_backward_workspace_bytes, gcs_segment_csr_*): the same launches, the same bits; the forward ignores its
 * workspace and gcs_subm_workspace_bytes_t reports 0 for it.
 *
 * GCS_F16: IEEE binary16.  The convolution has ONE engine, the matrix cores (v_mfma_f32_16x16x16_f16), and no chooser of
 * its own: its launch plan is gcs_subm_engine_plan(GCS_ENGINE_MFMA, n, cin, cout, kvol) -- the tiles of the forward and of
 * dX, their tap slices, the dW tile, the dW and dB slice counts -- so a test can assert which variant a shape reaches
 * without another query.  The engine of the `_engine` calls (and whatever a binding keeps as its default engine) does not
 * affect it.  Rows are cin (cout) halves long, any count, odd ones included.
 * Numerics: operands are read as binary16; every product is exact in fp32; accumulation is fp32, inside the matrix cores and
 * across taps, slices and chunks, in a fixed order; the bias is added in fp32 after the sum; y, dx, dw and db are rounded
 * to binary16 exactly ONCE, on the store (nearest even, overflow to +-inf as the conversion does).  With dups != 0 the fold
 * of dy onto the representatives is summed in fp32 and stored as binary16: one more rounding in what reads the fold (dx);
 * rows of one voxel still get identical outputs.  No float atomics: results are bit-identical from run to run.
 * Workspace: partial tiles and partial dw / db are fp32, the fold is binary16; gcs_subm_workspace_bytes_t reports the
 * sizes, which never exceed those of gcs_subm_engine_workspace_bytes(GCS_ENGINE_MFMA, ...) for the same shape; its
 * previous contents never matter; nothing is allocated and the host never waits.
 * segment_csr: sum and mean accumulate in fp32 in row order, mean divides in fp32, one rounding follows; min and max are
 * exact, `arg` is the FIRST row attaining the value, an empty segment gives 0 and arg -1.  Backward: sum copies bits, mean
 * is dout / count in fp32 rounded once, min and max route the bits to `arg`.
 * Errors, all GCS_ERR_INVALID_ARGUMENT before anything is queued: an unknown dtype; a workspace that is missing or too
 * small when the plan needs one; with GCS_F16 a typed pointer that is not 2-byte aligned, or a workspace that is not 4-byte
 * aligned (it holds fp32 partials).  The float entry points above do not check their workspace's alignment: it must be
 * 4-byte aligned there too. */
enum gcs_dtype { GCS_F32 = 0, GCS_F16 = 1 };
int gcs_dtypes(void); /* host only: bit (1 << dtype) for every dtype the library runs: 3 */
int gcs_subm_workspace_bytes_t(int32_t dtype, int64_t n, int32_t cin, int32_t cout, int32_t kvol, int32_t dups,
                               size_t* forward_bytes, size_t* backward_bytes);
int gcs_subm_forward_t(int32_t dtype, const void* rulebook, int64_t n, int32_t kvol, const void* features, int32_t cin,
                       const void* weight, const void* bias, int32_t cout, void* out,
                       void* workspace, size_t workspace_bytes, void* hip_stream);
int gcs_subm_backward_t(int32_t dtype, const void* rulebook, int64_t n, int32_t kvol, int32_t dups, const void* features,
                        int32_t cin, const void* weight, int32_t cout, const void* dout, void* dx, void* dw, void* db,
                        void* workspace, size_t workspace_bytes, void* hip_stream);
int gcs_segment_csr_forward_t(int32_t dtype, const void* src, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                              int32_t reduce, void* out, int64_t* arg, void* hip_stream);
int gcs_segment_csr_backward_t(int32_t dtype, const void* dout, int64_t m, int64_t f, const int64_t* indptr, int64_t s,
                               int32_t reduce, const int64_t* arg, void* dsrc, void* hip_stream);


/* Index plans of the point backbone.  GCS_ABI_VERSION stays 4, as for the typed entry points:
 * nothing existing changes, and gcs_index_orders() is how a binding learns whether the library has the plans.  The
 * library allocates nothing, everything runs on the caller's stream, and an argument error is GCS_ERR_INVALID_ARGUMENT
 * before anything is queued.
 *
 * gcs_serialize: what models/pt_v3.py's Point.serialization computes.  grid_coord int32 [n][3], batch int64 [n] or NULL,
 * orders_host the n_orders requested gcs_order values (HOST memory, each at most once); code, order, inverse int64
 * [n_orders][n], row r for orders_host[r].  The host never waits.
 *   codes    The four curve orders take a coordinate modulo 2^depth.  Z: bit i of x, y, z goes to bit 3i+2, 3i+1, 3i.
 *            HILBERT: Skilling's transform of the three axes, Gray step, interleave with axis 0 most significant.  The
 *            `_TRANS` orders swap x and y first.  CORD: (int64) trunc((float(x) / cord_div_x + float(y) / cord_div_y) +
 *            float(z)) in binary32 with IEEE division, coordinates as they are; for the reference's grid_size pass
 *            cord_div_x = (float)(grid_size * grid_size), cord_div_y = (float)grid_size.  With batch the code is
 *            batch << 3 * depth | code.
 *   order    order[r] sorts code[r] ascending as SIGNED int64, ties to the lower row (a stable sort), and
 *            inverse[r][order[r][j]] = j.
 *   refused  n outside 0...2^31-1, depth outside 1...16, n_batches < 1, 3 * depth + bit_length(n_batches) > 63, an unknown
 *            or repeated order, n_orders outside 1...5, a zero or NaN divisor, a workspace that is missing or smaller than
 *            gcs_serialize_workspace_bytes(n, n_orders) (0 with an error for arguments out of range); n == 0 does nothing.
 *
 * gcs_patch_plan_*: what SerializedAttention.get_padding_and_inverse computes from offset int64 [n_batches] (device,
 * inclusive row ends of the batches, non-decreasing) and the patch size P.  A batch of n_i rows is padded to
 * n_i > P ? ceil(n_i / P) * P : n_i rows; off_pad are the padded starts.  unpad[j] = j + off_pad[i] - off[i];
 * pad[p] = (p >= off_pad[i] + n_i ? p - P : p) - (off_pad[i] - off[i]); cu_seqlens lists every off_pad[i] + m * P below
 * off_pad[i + 1], in batch order, then the padded total.
 *   _count   one launch that writes counts_host[0] = padded rows and counts_host[1] = cu_seqlens entries, and the call's
 *            ONE wait for the stream.  counts_host must be pinned host memory (hipHostMalloc, a torch pinned tensor):
 *            the kernel writes it directly.
 *   _emit    fills pad [padded], unpad [offset[n_batches - 1]] and cu_seqlens [n_cu] for the counts _count reported;
 *            never waits.  Every store is held inside those lengths.  A batch's padded start is summed over the batches
 *            before it by the batch's own workgroups: meant for the hundreds of batches of a frame, not for millions.
 *   refused  n_batches < 1, patch_size < 1, a null pointer, counts_host that the device cannot write, padded beyond
 *            2^31-1 (cu_seqlens is int32), n_cu that no _count call can have reported. */
enum gcs_order { GCS_ORDER_CORD = 0, GCS_ORDER_Z = 1, GCS_ORDER_Z_TRANS = 2, GCS_ORDER_HILBERT = 3, GCS_ORDER_HILBERT_TRANS = 4 };
int gcs_index_orders(void); /* host only: bit (1 << order) for every order the library computes: 31 */
size_t gcs_serialize_workspace_bytes(int64_t n, int32_t n_orders);
int gcs_serialize(const int32_t* grid_coord, const int64_t* batch, int64_t n, int32_t n_batches, int32_t depth,
                  float cord_div_x, float cord_div_y, const int32_t* orders_host, int32_t n_orders, int64_t* code,
                  int64_t* order, int64_t* inverse, void* workspace, size_t workspace_bytes, void* hip_stream);
int gcs_patch_plan_count(const int64_t* offset, int32_t n_batches, int64_t patch_size, int64_t counts_host[2],
                         void* hip_stream);
int gcs_patch_plan_emit(const int64_t* offset, int32_t n_batches, int64_t patch_size, int64_t padded, int64_t n_cu,
                        int64_t* pad, int64_t* unpad, int32_t* cu_seqlens, void* hip_stream);

/* SerializedPooling / SerializedUnpooling of the point backbone.  GCS_ABI_VERSION stays 4:
 * nothing existing changes, and gcs_pool_reduces() is how a binding learns whether the library has these entry points.
 * The library allocates nothing, everything runs on the caller's stream, and an argument error is
 * GCS_ERR_INVALID_ARGUMENT before anything is queued.
 *
 * gcs_pool_plan_*: the cluster plan of models/pt_v3.py's SerializedPooling.forward, a function of the point set's
 * serialized_code alone.  code int64 [k][n] (device; k order rows), shift = 3 * pooling_depth.
 *   key        key[j] = code[0][j] >> shift (arithmetic).  Clusters are the distinct keys in ascending SIGNED order,
 *              numbered 0...S-1.
 *   cluster    int64 [n]: the number of row j's key (torch.unique(sorted=True, return_inverse=True)).
 *   idx_ptr    int64 [S + 1]: the exclusive scan of the cluster sizes, idx_ptr[S] = n.
 *   indices    int64 [n]: the rows sorted by cluster, ties to the LOWER row (torch.sort(cluster, stable=True)).
 *   head       int64 [S]: indices[idx_ptr[c]], the lowest row of cluster c.
 *   down_code  int64 [k][S]: code[r][head[c]] >> shift.
 *   down_order, down_inverse  int64 [k][S]: down_order[r] sorts down_code[r] ascending as signed int64 with ties to the
 *              lower position (gcs_serialize's rule), down_inverse[r][down_order[r][c]] = c.
 *   _count     sorts the keys, marks and counts the cluster heads, writes S to counts_host[0] and performs the call's ONE
 *              wait for the stream.  counts_host must be pinned host memory: a kernel writes it directly.  The workspace
 *              (gcs_pool_plan_workspace_bytes(n, k) bytes, 8-byte aligned) carries the sorted rows to _emit.
 *   _emit      with the same code, k, n, shift and workspace and the s that _count reported, fills the seven arrays; never
 *              waits.  Every store is held inside the lengths n, s + 1, s and k * s, so a workspace that does not belong
 *              to the call leaves a wrong plan, not a stray write.
 *   refused    n outside 1...2^31-1, k outside 1...5, shift outside 0...48 or no multiple of 3, a null pointer, a workspace
 *              that is missing or smaller than the query (0 with an error for arguments out of range), counts_host that
 *              the device cannot write, s outside 1...n.
 *
 * gcs_segment_gather_forward_t: out[c][ch] = reduce over j in [indptr[c], indptr[c + 1]) of src[indices[j]][ch].
 * src [m][f] of `dtype` with a row stride of src_stride elements (>= f), indices int64 [m], indptr int64 [s + 1] (entries
 * are clamped to [0, m]), out [s][f] dense.  The numerics are segment_csr's: sum and mean are ONE fp32 chain in ascending
 * j, mean divides in fp32, one rounding on the store; min and max compare exactly and copy bits; an empty segment gives 0.
 * arg int64 [s][f] (required for min and max, unused otherwise and may be NULL) receives the SOURCE row indices[j] of the
 * first j that attains the value, -1 for an empty segment.  The result is segment_csr(src[indices], indptr) bit for bit.
 * An entry of indices outside [0, m) is skipped.
 *
 * gcs_segment_gather_backward_t: the transpose, by row: with g = dout[cluster[r]][ch], dsrc[r][ch] = g (sum), g / count
 * in fp32 rounded once (mean), arg[cluster[r]][ch] == r ? g : 0 (min, max).  dout [s][f] dense, dsrc [m][f] with a row
 * stride of dsrc_stride elements.  Every element of dsrc is written exactly once: nothing is cleared first, there are no
 * atomics, and the result is bit-identical from run to run.  PRECONDITION, not checked on the device: cluster int64 [m]
 * and indptr come from ONE plan, and every row is in exactly one segment (a cluster entry outside [0, s) gives a zero row).
 *
 * gcs_segment_expand_add_t: out[r] = a[r] + b[cluster[r]], one fp32 add rounded once; a may be NULL (out[r] =
 * b[cluster[r]]).  a and out [m][f], b [rows][f], all dense.  PRECONDITION: every cluster entry is a row of b.  Its
 * transpose needs no kernel of its own: d_a = dout, d_b = gcs_segment_gather_forward_t(dout, indices, idx_ptr, GCS_SUM).
 *
 * The three take 16-byte pieces of a row where f, the strides and the base addresses are multiples of 16 bytes, and single
 * elements otherwise.  Refused: an unknown dtype or reduce, m, s or f outside 1...2^31-1, a stride below f, a null pointer,
 * a typed pointer that is not aligned to its element or an index pointer that is not 8-byte aligned. */
int gcs_pool_reduces(void); /* host only: bit (1 << reduce) for every gcs_reduce the gathered reduce runs: 15 */
size_t gcs_pool_plan_workspace_bytes(int64_t n, int32_t k);
int gcs_pool_plan_count(const int64_t* code, int32_t k, int64_t n, int32_t shift, void* workspace, size_t workspace_bytes,
                        int64_t counts_host[1], void* hip_stream);
int gcs_pool_plan_emit(const int64_t* code, int32_t k, int64_t n, int32_t shift, int64_t s, void* workspace,
                       size_t workspace_bytes, int64_t* cluster, int64_t* indices, int64_t* idx_ptr, int64_t* head,
                       int64_t* down_code, int64_t* down_order, int64_t* down_inverse, void* hip_stream);
int gcs_segment_gather_forward_t(int32_t dtype, const void* src, int64_t src_stride, int64_t m, int64_t f,
                                 const int64_t* indices, const int64_t* indptr, int64_t s, int32_t reduce, void* out,
                                 int64_t* arg, void* hip_stream);
int gcs_segment_gather_backward_t(int32_t dtype, const void* dout, int64_t m, int64_t f, const int64_t* cluster,
                                  const int64_t* indptr, int64_t s, int32_t reduce, const int64_t* arg, void* dsrc,
                                  int64_t dsrc_stride, void* hip_stream);
int gcs_segment_expand_add_t(int32_t dtype, const void* a, const void* b, const int64_t* cluster, int64_t m, int64_t f,
                             void* out, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
