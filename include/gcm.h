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
 *
 * ---- The feed-forward third of a PTv3 Block (models/pt_v3.py, Block.forward's tail) -------------
 * For N rows, C channels and Hd hidden features, all float32:
 *     mean_r = (1/C) sum_c x_rc;  var_r = (1/C) sum_c (x_rc - mean_r)^2;  rstd_r = 1 / sqrt(var_r + eps)
 *     xn = (x - mean) rstd ln_w + ln_b          torch.nn.LayerNorm (biased variance)
 *     a  = xn W1^T + b1                         w1 [Hd][C], b1 [Hd], contiguous
 *     g  = a (1 + erf(a / sqrt 2)) / 2          torch.nn.GELU(approximate='none')
 *     t  = g W2^T + b2                          w2 [C][Hd], b2 [C], contiguous
 *     y  = x + s_r t                            row_scale s: float [N] or NULL (NULL: y = x + t)
 *   C and Hd are positive multiples of 4, C <= gcm_ffn_max_channels() and Hd <= 4 gcm_ffn_max_channels(); N >= 0.
 *   x, y, dy, dx are row-strided under the rule above (width C); ln_w, ln_b [C]; every float pointer but row_scale
 *   (4-byte aligned) is 16-byte aligned.
 *
 * gcm_ffn_max_channels (host only): the largest C the fused kernels run, 128 in this build; never 0.  A binding asks
 *     it to learn that the library has the operator and which widths go to it.
 * gcm_ffn_forward: one launch.  a == NULL (inference): the hidden tensor never reaches memory; mean and rstd may then
 *     be NULL too (both or neither).  a != NULL: the pre-activation a [N][Hd] is stored once and mean, rstd [N] beside
 *     it, for the backward.  N == 0 returns 0 and queues nothing.
 * gcm_ffn_backward: from the stored mean, rstd and a (read, never written: the call may be repeated),
 *     dt = s_r dy;  dg = dt W2;  da = dg (Phi(a) + a phi(a));  dxn = da W1;
 *     dx = dy + rstd (u - mean_c(u) - xhat mean_c(u xhat)),  u = dxn ln_w,  xhat = (x - mean) rstd;
 *     dln_w = sum_r dxn xhat;  dln_b = sum_r dxn;  dw1 [Hd][C] = da^T xn;  db1 = sum_r da;  dw2 [C][Hd] = dt^T g;
 *     db2 = sum_r dt.
 *     ln_b is an input of the backward because dw1 is taken against xn, which holds it.  Every output is written
 *     whole, a NULL output is skipped.  workspace is gcm_ffn_backward_workspace_bytes(N, C, Hd) bytes (never 0 for
 *     arguments in range), 256-byte aligned; what it held before does not matter.
 *
 * Rounding and order: the LayerNorm sums are fp32; four lanes own a row, lane q adds its elements 4 q + 16 k .. + 3 in
 * ascending order from 0 and the four lanes are added as (q0 + q1) + (q2 + q3); mean and var are the sums divided by
 * C, rstd is 1 / sqrt with IEEE division and square root.  Every matrix product runs on v_mfma_f32_16x16x4_f32: a and
 * dg are one fp32 chain from 0 over the channels in ascending order; t and dxn are, per chunk of 64 hidden features
 * (ascending), one chain from 0 over the chunk, and the chunks' results are added in ascending order; b1, b2 are
 * added after the chains; s_r t is one fp32 product, then one fp32 add of x -- a row with s_r = 0 has y == x and
 * dx == dy bit for bit (finite t).  erf and exp are the device library's float32 functions.  No float atomics: dw1,
 * db1, dw2, db2 are sums over at most 64 row slices added pairwise (a fixed tree: slice s + w to slice s for w = 1, 2,
 * 4 .. 32, a slice that does not exist counting as 0); inside a slice every 32 consecutive rows are one chain
 * from 0 in ascending row order (for db1, db2 four rows a chain, four chains paired as (0 + 1) + (2 + 3) per 16 rows,
 * the 16-row sums chained) and the 32-row sums are added in ascending order; dln_w, dln_b are sums over tiles of 64
 * rows (inside a tile, groups of CT / 16 consecutive rows in ascending order, CT = 32, 64 or 128 the smallest that
 * holds C), the tiles added in ascending order, in groups of consecutive tiles when there are more than 64.  The
 * slices and groups depend on N, C and Hd alone: every output is bit-identical from run to run and independent of
 * how many workgroups the device holds at a time.
 *
 * The same operator up to 512 channels, the hidden width split across workgroups (gcm_ffn_split_*).  C <=
 * gcm_ffn_split_max_channels() (512 in this build) and Hd <= 4 times that; every other argument rule is the one above.
 * gcm_ffn_split_plan (host only) tells how the row side runs, a function of N, C and Hd alone: in split mode (tiles x
 *     chunks <= plan[6]) every (tile of 64 rows, chunk of 64 hidden features) pair has a workgroup of its own and leaves
 *     its t (backward: dxn) as one of P = ceil(Hd / 64) partial records [N][C]; in rows mode a workgroup walks all chunks
 *     of its tile and leaves one record, so that the workspace stays bounded.
 * gcm_ffn_split_workspace_bytes (host only): the bytes of the forward's and of the backward's workspace (a NULL
 *     pointer is skipped), never 0 for arguments in range; the forward's holds P N C floats.
 * gcm_ffn_split_forward: two launches, gcm_ffn_forward's arguments and a workspace (256-byte aligned; what it held
 *     before does not matter).  N == 0 returns 0 and queues nothing.
 * gcm_ffn_split_backward: gcm_ffn_backward's arguments unchanged, the workspace sized by the query above.
 * Rounding and order: as above, with CT = 32, 64, 128, 256 or 512 the smallest that holds C.  The partial records are
 * added in ascending chunk order from +0, then b2, s_r and x as above (backward: then the LayerNorm backward), which is
 * the order the one-launch kernels add their chunks in registers: the mode never shows in the bits, and for C <= 128
 * every output of the split entry points has the bits of gcm_ffn_forward / gcm_ffn_backward.  At CT = 256 and 512 the
 * LayerNorm backward forms xhat and u twice (once for the row's two sums, once for dx) by the same operations; each
 * lane's sums keep their element order, and a tile's column sums are over groups of 16 and 32 consecutive rows.
 *
 * ---- The front of a PTv3 Block (models/pt_v3.py, Block.forward between the sparse convolution and the attention;
 * DESIGN.md section 19) ---------------------------------------------------------------------------------------------------
 * For N rows, C channels and O projected features, all float32:
 *     t    = s Wc^T + bc                        s [N][C] the convolution's output, wc [C][C], bc [C]   (cpe[1])
 *     u    = that lnc_w + lnc_b                 that = (t - mean_c) rstd_c, eps_c                       (cpe[2])
 *     feat = x + u                              x [N][C] the Block's shortcut                           -> output 1
 *     n    = fhat ln1_w + ln1_b                 fhat = (feat - mean_1) rstd_1, eps_1                    (norm1)
 *     qkv  = n Wq^T + bq                        wq [O][C], bq [O]                                       -> output 2
 *   mean and rstd as above (biased variance).  C and O are positive multiples of 4, C <= gcm_front_max_channels() and
 *   O <= 3 gcm_front_max_channels(); N >= 0.  x, s, feat, qkv, dfeat, dqkv, dx, ds are row-strided under the rule above
 *   (width C, or O for qkv and dqkv); the parameters, t [N][C] and the statistics [N] are contiguous; every float pointer
 *   but the four statistics (4-byte aligned) is 16-byte aligned.
 *
 * gcm_front_max_channels (host only): the largest C the fused kernels run, 128 in this build; never 0.
 * gcm_front_forward: one launch.  t == NULL (inference): nothing but feat and qkv reaches memory and the four statistics
 *     are NULL too.  t != NULL: the pre-norm product t and mean_c, rstd_c, mean_1, rstd_1 are stored once for the
 *     backward; all four are then required.  N == 0 returns 0 and queues nothing.
 * gcm_front_backward: from the stored s, feat, t and statistics (read, never written: the call may be repeated) and the
 *     two gradients dfeat [N][C] and dqkv [N][O], both required,
 *     dn = dqkv Wq;  df = dfeat + rstd_1 (v - mean_c(v) - fhat mean_c(v fhat)), v = dn ln1_w;  dx = df;
 *     dt = rstd_c (w - mean_c(w) - that mean_c(w that)), w = df lnc_w;  ds = dt Wc;
 *     dwq [O][C] = dqkv^T n;  dbq = sum_r dqkv;  dwc [C][C] = dt^T s;  dbc = sum_r dt;
 *     dln1_w = sum_r dn fhat;  dln1_b = sum_r dn;  dlnc_w = sum_r df that;  dlnc_b = sum_r df.
 *     ln1_b is an input because dwq is taken against n, which holds it.  Every output is written whole, a NULL output is
 *     skipped.  workspace is gcm_front_backward_workspace_bytes(N, C, O) bytes (never 0 for arguments in range), 256-byte
 *     aligned; what it held before does not matter.  Four launches, five when N is beyond 64 tiles of 64 rows.
 *
 * Rounding and order: every product of two matrices runs on v_mfma_f32_16x16x4_f32.  t, qkv and ds are one fp32 chain
 * from 0 over the channels in ascending order, bc / bq added after the chain; dn is, per chunk of 64 outputs (ascending),
 * one chain from 0 over the chunk, the chunks' results added in ascending order.  The LayerNorm sums follow the
 * feed-forward's four-lanes-per-row rule above, forward and backward; u is evaluated as
 * ((t - mean_c) rstd_c) lnc_w + lnc_b with one rounding per operation, and feat = x + u is one fp32 add.  No float
 * atomics: dwq, dbq, dwc, dbc are sums over at most 64 row slices added in the feed-forward's pairwise tree, inside a
 * slice every 32 consecutive rows one chain (the bias sums as db1 / db2 above); the four LayerNorm gradients are sums
 * over tiles of 64 rows (inside a tile as dln_w above), the tiles added in ascending order, in groups of consecutive
 * tiles when there are more than 64.  Slices and groups depend on N, C and O alone: every output is bit-identical from
 * run to run and independent of how many workgroups the device holds at a time.
 *
 * ---- The middle of a PTv3 Block (models/pt_v3.py, SerializedAttention.forward around its attention, and the Block's
 * DropPath and residual add after it) ---------------------------------------------------------------
 * For N rows (points), T >= N slots (padded patch positions), C channels, float32 data, int64 indices as torch has them:
 *     order [T]    slot -> row            (serialized_order[i][pad])
 *     inverse [N]  row -> its own slot    (unpad[serialized_inverse[i]])
 *     extra [N]    int32: the row's duplicate slot, or -1
 *   PRECONDITION of every data function below: order[inverse[n]] == n for every row, and at most one slot j per row with
 *   order[j] == n and inverse[n] != j (the duplicate slot: a row of the previous patch borrowed to fill the last one;
 *   get_padding_and_inverse borrows from one patch, so a row is borrowed at most once).  The functions do not verify it;
 *   with it, every sum below has at most two terms and every output element exactly one writer.  An index that is
 *   negative, or not below the range the function knows (N for order in gcm_mid_slot_plan, T for inverse and extra in
 *   gcm_mid_backward), is not dereferenced: the row is skipped.
 *     gather            y[j] = x[order[j]]                               x [.][W], y [T][W]
 *     its gradient      dx[n] = dy[inverse[n]] + dy[extra[n]]            the second term when extra[n] >= 0; one fp32 add
 *     p = a[inverse[n]] Wp^T + bp                                        a [T][C] the attention's output, wp [C][C], bp [C]
 *     y = x + p, or y = x + (p r[n])                                     x [N][C] the shortcut, r = row_scale [N] or NULL
 *   x, a, y, dy are row-strided under the rule above; the gather's y and dx ([T][W], [N][W]), da [T][C] and the parameters
 *   are contiguous.  Float pointers are 16-byte aligned (row_scale 4-byte), order and inverse 8-byte, extra 4-byte.  W and C
 *   are positive multiples of 4, C <= gcm_mid_max_channels(); N and T are refused at 2^31 and above, T < N is refused.
 *   No call waits for the device; a NULL output is skipped.
 *
 * gcm_mid_max_channels (host only): the largest C the fused kernels run, 128 in this build; never 0.
 * gcm_mid_slot_plan: extra from order and inverse; two launches, integer stores only.
 * gcm_mid_gather_forward, gcm_mid_gather_backward: one launch each, 16-byte copies; every element of y / dx is written
 *     exactly once.  A two-term fp32 sum is commutative: dx has the bits of torch's index_put_(accumulate=True).
 * gcm_mid_forward: one launch.  p is one fp32 chain from 0 over the channels in ascending order on v_mfma_f32_16x16x4_f32,
 *     bp added after the chain; p r[n] is one multiply and x + . one add, not contracted.
 * gcm_mid_backward: with g = r o dy (recomputed where needed, never stored; dy is only read: the call may be repeated),
 *     da [T][C]: row inverse[n] = g[n] Wp (one chain over the channels), row extra[n] = exact zeros: written whole;
 *     dwp [C][C] = g^T a[inverse];  dbp = sum_n g[n]: sums over at most 64 row slices added in the feed-forward's pairwise
 *     tree, inside a slice every 32 consecutive rows one chain (the bias sums as db1 / db2 above).  No float atomics.
 *     The gradient of the shortcut x is dy itself and is not computed.  workspace is
 *     gcm_mid_backward_workspace_bytes(N, C) bytes (never 0 for arguments in range), 256-byte aligned; what it held before
 *     does not matter.  One launch for da, two for dwp / dbp, whatever N is.  The slices depend on N and C alone: every
 *     output is bit-identical from run to run and independent of how many workgroups the device holds at a time.
 *
 * ---- The seams between the PTv3 stages (models/pt_v3.py: Embedding.stem's tail, SerializedPooling's norm / act,
 * SerializedUnpooling.proj and proj_skip) -------------------------------------------------------------
 * Linear -> BatchNorm1d -> GELU as one operator, for N rows, I inputs, O outputs, float32:
 *     z = x W^T + b                      w [O][I] contiguous, b [O] or NULL;  w == NULL: z is x itself and I == O
 *     batch statistics (training)        mean_c = (1/N) sum_r z_rc;  var_c = (1/N) sum_r (z_rc - mean_c)^2
 *     running statistics (eval)          mean_c = running_mean_c;  var_c = running_var_c
 *     rstd = 1 / sqrt(var + eps);  u = ((z - mean) rstd) g + h             g, h = bn_w, bn_b [O]
 *     y = act ? u (1 + erf(u / sqrt 2)) / 2 : u
 *     training also: running_mean = (1 - m) running_mean + m mean;  running_var = (1 - m) running_var + m var N / (N - 1);
 *     num_batches_tracked += 1
 *   x, y, dy and dx are row-strided under the rule above; z is [N][O] contiguous where the library writes it and carries a
 *   stride where it reads it (with w == NULL the caller passes x and its stride as z).  Float pointers are 16-byte aligned,
 *   the int64 counter 8-byte.  I and O are positive multiples of 4, at most gcm_seam_max_channels(); N is refused at 2^31
 *   and above; w == NULL with I != O is refused, as are b, z, dw or db without w.  Training refuses N == 1 (torch raises
 *   there); with N == 0 the forwards queue nothing and the backward queues only the clears of the parameter gradients
 *   asked for.  Arguments are checked before anything is queued; no call allocates or waits.
 *
 * gcm_seam_max_channels (host only): the largest I and O, 512 in this build; never 0.
 * gcm_seam_forward_eval: ONE launch; nothing but y reaches memory unless z [N][O] or rstd [O] is given (a caller that wants a
 *     gradient in eval mode gives both).  z is one fp32 chain from 0 over the inputs in ascending order on
 *     v_mfma_f32_16x16x4_f32 -- the accumulators carry across the chunks of 128 inputs staged at a time -- and b is added
 *     after the chain.  rstd = 1 / sqrt(var + eps) with IEEE division and square root; u is a subtraction, two multiplies
 *     and an add in the order written above, not contracted.  With w == NULL the launch is elementwise.
 * gcm_seam_forward_train: three launches whatever N is.  (1) the product stores z and, per tile of 64 rows and column, the
 *     tile's mean over its valid rows in ascending order, taken about the tile's first row (z0 + sum (z - z0) / n: a column
 *     whose mean is many standard deviations keeps its digits), and, about that mean, the centred second moment M2 (with
 *     w == NULL this launch only reads x).  (2) per column the tiles' (count, mean, M2) are merged in ascending tile order
 *     with the parallel-variance merge -- sum z^2 - (sum z)^2 / N is never formed -- beyond 64 tiles in at most 64 groups of
 *     consecutive tiles, each merged in order, the groups then merged in ascending order; the mean itself is a compensated
 *     (Kahan) sum of count_t mean_t in the same order divided by N, as the tile's mean is one of z - z0; this launch
 *     writes mean and rstd [O] and, when the three buffers are given (all or none), the running statistics and the counter, plain stores from
 *     one thread per column.  (3) y from z in 16-byte accesses.  workspace is gcm_seam_forward_workspace_bytes(N, O) bytes
 *     (never 0 for arguments in range), 256-byte aligned; what it held before does not matter.
 * gcm_seam_backward: from x, z, mean, rstd and dy, all only read: the call may be repeated.  batch_stats says whether mean
 *     and rstd were the batch's.  With zhat = (z - mean) rstd and u = zhat g + h recomputed from z:
 *       du = act ? dy (Phi(u) + u phi(u)) : dy;  dbn_b = sum_r du;  dbn_w = sum_r du zhat
 *       dz = (g rstd) (du - dbn_b / N - zhat dbn_w / N) under batch statistics, dz = (g rstd) du under running ones
 *       dx = dz W;  dw [O][I] = dz^T x;  db = sum_r dz
 *     dbn_b and dbn_w: per tile of 64 rows four chains of 16 rows added in order, the tiles added in ascending order, beyond
 *     64 tiles in groups as the statistics; two launches, and none under running statistics when neither is asked for.
 *     dx: one launch; dz is staged in LDS per 64 rows and never stored.  dx is, per chunk of 128 outputs, one fp32 chain
 *     from 0 over the chunk's outputs in ascending order, and the chunks' results are added in ascending order (O <= 128:
 *     one chain).  dw and db: sums over at most 64 row slices added in the feed-forward's pairwise tree, inside a slice
 *     every 32 consecutive rows one chain (the bias sums as db1 / db2 above); two launches.  Five launches under batch
 *     statistics whatever N is; no float atomics.  Every output is written whole; a NULL output is skipped and skips its
 *     launches.  With w == NULL dx is dz (one elementwise launch) and there is no dw or db.  workspace is
 *     gcm_seam_backward_workspace_bytes(N, I, O) bytes, 256-byte aligned.  Slices and groups depend on N, I and O alone:
 *     every output is bit-identical from run to run and independent of how many workgroups the device holds at a time.
 *
 * ---- The attribute head at inference in one launch per output key --------------------------------
 * For N rows, I input features, K class columns, H hidden features and C = 1 or 3 outputs, all float32, g = group[r]
 * (group == NULL: every row has g = 0):
 *     f   = leaky(x[r] W1^T + onehots[r] Wma^T + b1)          w1 [H][I] row stride w1_stride, b1 [H], w_ma [H][K] contiguous
 *     h   = leaky((f o alpha[g]) W2^T + beta[g] + bias2)      w2 [H][H] row stride w2_stride; alpha, beta [G][H], bias2 [H]
 *     out = T(h Wout^T + bout)                                w_out [C][H] contiguous, b_out [C]; T by gcm_kind as gcm_head_out
 *   alpha, beta, bias2 and b_out may each be NULL (ones, zeros, zeros, zeros): a plain Linear is alpha = beta = NULL with
 *   bias2 its bias, a ModLinear(output_mode, mod_bias, bias=None) is alpha and beta with bias2 = NULL.  A row whose group is
 *   outside 0 .. G-1 gives exact zeros.  I and H are positive multiples of 4, I <= gcm_head_chain_max_in() (256 in this
 *   build) and H <= gcm_head_chain_max_hidden() (512); 1 <= K <= 32.  x is row-strided under the rule above; onehots is
 *   dense float32 [N][K] of ANY values with a row stride in elements of at least K, 4-byte aligned; every other float
 *   pointer is 16-byte aligned.  out is contiguous [N][C].  slope is finite and > 0, factor finite.
 * gcm_head_chain: one launch, no workspace; neither f nor h reaches memory.  N == 0 returns 0 and queues nothing.  Every
 *     product runs on v_mfma_f32_16x16x4_f32: f is one fp32 chain from 0 over x's features in ascending order (I rounded
 *     up to 16 with zeros) and then over the K class columns, b1 added after the chain; h is one chain over H, then beta,
 *     then bias2; out is, per row and per quarter (64 columns) of every chunk of 256 columns, 16 lanes that each chain fmaf
 *     over their columns (lane l: l, l + 16, l + 32, l + 48 of the quarter) over the chunks in ascending order, added by a
 *     fixed exchange tree (lanes 8, 4, 2, 1 apart), the four quarters in ascending order, then b_out; T in double, rounded
 *     once.  No float atomics: a row's bits depend on that row's inputs and the parameters alone -- not on N, the row's
 *     position or the run.  The kernel needs up to 157 184 bytes of LDS, which it asks the runtime for on the first call;
 *     a refusal comes back as GCM_ERR_HIP with the text.
 *
 * ---- The head's output layers in a training step ----------------------------------------------------
 * Up to four keys (gcm_kind: xyz, rgb, scale, opacity), each at most once, in the caller's order, over the same N rows and
 * the same hidden width I (a positive multiple of 4, at most gcm_head_train_max_in(): 512 in this build).  A key is a
 * gcm_head_key: h [N][I] row-strided under the rule above, w [C][I] contiguous with C = 1 for opacity and 3 otherwise,
 * b [C] or NULL, factor finite; h, w, dh and dw are 16-byte aligned, out / dout have a row stride of at least C elements.
 * group is int32 [N] or NULL; only "group[r] >= 0" matters, as in gcm_head_out.
 *     pre = h[r] . w[c] + b[c]                       gcm_head_out's summation, so out has gcm_head_out's bits
 *     out = T(pre) by kind, exact zeros for a row without a group
 * gcm_head_train_forward: ONE launch whatever n_keys is.  The values go EITHER to every key's out (points14 == NULL) OR to
 *     points14, contiguous [N][14], the rasterizer's record (every key's out == NULL; needs the rgb key, xyz and scales,
 *     [N][>= 3] with row strides in elements, read and never written):
 *         0..2  xyz + out.xyz (xyz without the key)     3  out.opacity (1 without the key)
 *         4..6  scales * out.scale (scales without it)  7..10  1, 0, 0, 0     11..13  out.rgb
 *     in float32 on the bits above.  pre, when not NULL, is [N][gcm_head_train_pre_floats()] float32 and receives pre at
 *     columns 3 * kind + c: what the backward reads.  N == 0 returns 0 and queues nothing (out, points14 and dout may
 *     then all be NULL).
 * gcm_head_train_backward: the incoming gradient is EITHER every key's dout [N][C] (dpoints14 == NULL) OR dpoints14
 *     [N][>= 14] with row stride dpoints_stride as the rasterizer's node returns it (every key's dout == NULL; the scale
 *     key's dout is then dpoints14[r][4..6] * scales[r], so scales is needed with that key).
 *         dv = dout * factor * s (1 - s), s = sigmoid(pre) in double, rounded once         xyz, rgb, opacity
 *         dv = dout * factor where -1 <= pre <= 1 (both ends included), else 0            scale
 *         dv = 0 for a row without a group: an exact zero row of dh, no term in dw / db
 *         dh [N][I] (row stride dh_stride) = dv w      dw [C][I] = dv^T h      db [C] = sum over the rows of dv
 *     Two launches whatever N and n_keys are, no float atomics; each output is written whole by plain stores, a NULL
 *     output is skipped, inputs are never written.  workspace is gcm_head_train_workspace_bytes(N, I, n_keys) bytes,
 *     256-byte aligned, and need not be cleared.  N == 0 writes zeros to dw / db.  The row blocks, their records and the
 *     fold's groups are gcm_head_train_plan's, a function of N and I alone: every output is bit-identical from run to
 *     run, on any stream.
 * gcm_head_train_plan fills plan[0..7]: tiles of 64 rows, tiles per row block, row blocks (= records per key), first-level
 *     groups of the fold, records per group, fold levels (1 or 2), floats between records, floats between the keys' blocks.
 * Refused with GCM_ERR_INVALID_ARGUMENT and a message before anything is queued: an unknown or repeated kind, n_keys
 *     outside 1..4, I not a positive multiple of 4 or above the limit, a bad stride or alignment, neither or both
 *     output / gradient forms, the [N][14] form without rgb, xyz or scales, a workspace that is too small.
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

int gcm_ffn_max_channels(void);

int gcm_ffn_forward(const float* x, int64_t x_stride, const float* ln_w, const float* ln_b, float eps, const float* w1,
                    const float* b1, const float* w2, const float* b2, const float* row_scale, int64_t N, int32_t C,
                    int32_t Hd, float* y, int64_t y_stride, float* mean, float* rstd, float* a, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_ffn_backward_workspace_bytes(int64_t N, int32_t C, int32_t Hd);

int gcm_ffn_backward(const float* x, int64_t x_stride, const float* mean, const float* rstd, const float* a,
                     const float* dy, int64_t dy_stride, const float* row_scale, const float* ln_w, const float* ln_b,
                     const float* w1, const float* w2, int64_t N, int32_t C, int32_t Hd, float* dx, int64_t dx_stride,
                     float* dln_w, float* dln_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                     size_t workspace_bytes, void* hip_stream);

int gcm_ffn_split_max_channels(void);

/* plan[0] mode (0 rows, 1 split), [1] row tiles, [2] hidden chunks, [3] partial records P, [4] weight-gradient slices,
   [5] first-level LayerNorm groups, [6] the tiles x chunks limit, [7] 0 */
int gcm_ffn_split_plan(int64_t N, int32_t C, int32_t Hd, int64_t plan[8]);

int gcm_ffn_split_workspace_bytes(int64_t N, int32_t C, int32_t Hd, size_t* forward_bytes, size_t* backward_bytes);

int gcm_ffn_split_forward(const float* x, int64_t x_stride, const float* ln_w, const float* ln_b, float eps, const float* w1,
                          const float* b1, const float* w2, const float* b2, const float* row_scale, int64_t N, int32_t C,
                          int32_t Hd, float* y, int64_t y_stride, float* mean, float* rstd, float* a, void* workspace,
                          size_t workspace_bytes, void* hip_stream);

int gcm_ffn_split_backward(const float* x, int64_t x_stride, const float* mean, const float* rstd, const float* a,
                           const float* dy, int64_t dy_stride, const float* row_scale, const float* ln_w, const float* ln_b,
                           const float* w1, const float* w2, int64_t N, int32_t C, int32_t Hd, float* dx, int64_t dx_stride,
                           float* dln_w, float* dln_b, float* dw1, float* db1, float* dw2, float* db2, void* workspace,
                           size_t workspace_bytes, void* hip_stream);

int gcm_front_max_channels(void);

int gcm_front_forward(const float* x, int64_t x_stride, const float* s, int64_t s_stride, const float* wc, const float* bc,
                      const float* lnc_w, const float* lnc_b, float eps_c, const float* ln1_w, const float* ln1_b,
                      float eps_1, const float* wq, const float* bq, int64_t N, int32_t C, int32_t O, float* feat,
                      int64_t feat_stride, float* qkv, int64_t qkv_stride, float* t, float* mean_c, float* rstd_c,
                      float* mean_1, float* rstd_1, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_front_backward_workspace_bytes(int64_t N, int32_t C, int32_t O);

int gcm_front_backward(const float* s, int64_t s_stride, const float* feat, int64_t feat_stride, const float* t,
                       const float* mean_c, const float* rstd_c, const float* mean_1, const float* rstd_1,
                       const float* dfeat, int64_t dfeat_stride, const float* dqkv, int64_t dqkv_stride, const float* wc,
                       const float* lnc_w, const float* ln1_w, const float* ln1_b, const float* wq, int64_t N, int32_t C,
                       int32_t O, float* dx, int64_t dx_stride, float* ds, int64_t ds_stride, float* dwc, float* dbc,
                       float* dlnc_w, float* dlnc_b, float* dln1_w, float* dln1_b, float* dwq, float* dbq, void* workspace,
                       size_t workspace_bytes, void* hip_stream);

int gcm_mid_max_channels(void);

int gcm_mid_slot_plan(const int64_t* order, int64_t T, const int64_t* inverse, int64_t N, int32_t* extra, void* hip_stream);

int gcm_mid_gather_forward(const float* x, int64_t x_stride, const int64_t* order, int64_t T, int32_t W, float* y,
                           void* hip_stream);

int gcm_mid_gather_backward(const float* dy, int64_t dy_stride, const int64_t* inverse, const int32_t* extra, int64_t N,
                            int32_t W, float* dx, void* hip_stream);

int gcm_mid_forward(const float* a, int64_t a_stride, const int64_t* inverse, const float* x, int64_t x_stride,
                    const float* wp, const float* bp, const float* row_scale, int64_t N, int32_t C, float* y,
                    int64_t y_stride, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_mid_backward_workspace_bytes(int64_t N, int32_t C);

int gcm_mid_backward(const float* a, int64_t a_stride, const int64_t* inverse, const int32_t* extra, const float* dy,
                     int64_t dy_stride, const float* wp, const float* row_scale, int64_t N, int64_t T, int32_t C,
                     float* da, float* dwp, float* dbp, void* workspace, size_t workspace_bytes, void* hip_stream);

int gcm_seam_max_channels(void);

int gcm_seam_forward_eval(const float* x, int64_t x_stride, const float* w, const float* b, const float* running_mean,
                          const float* running_var, float eps, const float* bn_w, const float* bn_b, int act, int64_t N,
                          int32_t I, int32_t O, float* y, int64_t y_stride, float* z, float* rstd, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_seam_forward_workspace_bytes(int64_t N, int32_t O);

int gcm_seam_forward_train(const float* x, int64_t x_stride, const float* w, const float* b, float eps, float momentum,
                           const float* bn_w, const float* bn_b, int act, int64_t N, int32_t I, int32_t O, float* z, float* y,
                           int64_t y_stride, float* mean, float* rstd, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, void* hip_stream);

/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_seam_backward_workspace_bytes(int64_t N, int32_t I, int32_t O);

int gcm_seam_backward(const float* x, int64_t x_stride, const float* z, int64_t z_stride, const float* mean,
                      const float* rstd, const float* dy, int64_t dy_stride, const float* w, const float* bn_w,
                      const float* bn_b, int act, int batch_stats, int64_t N, int32_t I, int32_t O, float* dx,
                      int64_t dx_stride, float* dw, float* db, float* dbn_w, float* dbn_b, void* workspace,
                      size_t workspace_bytes, void* hip_stream);

int gcm_head_chain_max_hidden(void);
int gcm_head_chain_max_in(void);
int gcm_head_chain(const float* x, int64_t x_stride, const float* onehots, int64_t onehots_stride, const float* w1,
                   int64_t w1_stride, const float* b1, const float* w_ma, const float* w2, int64_t w2_stride,
                   const float* alpha, const float* beta, const float* bias2, const int32_t* group, const float* w_out,
                   const float* b_out, int64_t N, int32_t I, int32_t K, int32_t H, int32_t G, int32_t C, int kind,
                   float factor, float slope, float* out, void* hip_stream);

/* one key of gcm_head_train_*: strides in elements */
typedef struct gcm_head_key {
  int32_t kind; /* enum gcm_kind */
  float factor;
  const float* h;
  int64_t h_stride;
  const float* w;
  const float* b;
  float* out; /* forward, per-key form */
  int64_t out_stride;
  const float* dout; /* backward, per-key form */
  int64_t dout_stride;
  float* dh; /* backward outputs, each may be NULL */
  int64_t dh_stride;
  float* dw;
  float* db;
} gcm_head_key;

int gcm_head_train_max_in(void);
int gcm_head_train_pre_floats(void);
int gcm_head_train_plan(int64_t N, int32_t I, int64_t* plan);
/* 0 with a message in gcm_last_error() when an argument is out of range */
size_t gcm_head_train_workspace_bytes(int64_t N, int32_t I, int32_t n_keys);
int gcm_head_train_forward(const gcm_head_key* keys, int32_t n_keys, const int32_t* group, int64_t N, int32_t I, float* pre,
                           const float* xyz, int64_t xyz_stride, const float* scales, int64_t scales_stride,
                           float* points14, void* hip_stream);
int gcm_head_train_backward(const gcm_head_key* keys, int32_t n_keys, const int32_t* group, int64_t N, int32_t I,
                            const float* pre, const float* scales, int64_t scales_stride, const float* dpoints14,
                            int64_t dpoints_stride, void* workspace, size_t workspace_bytes, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
