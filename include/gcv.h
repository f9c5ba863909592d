/*
 * gcv.h -- C ABI of the MI355X-native point-generation / visibility path (libgcv_hip.so).
 *
 * the step immediately before the rasterizer in GaussianCity's
 * inference and dataset generation -- BEV maps -> extruded points -> voxel volume -> per-pixel
 * first-hit point id (scripts/dataset_generator.py:1251-1461).  Reference interfaces replaced:
 *
 *   gcv_extrude_count / gcv_extrude_emit   footprint_extruder.get_points_from_projection
 *                                          (extensions/footprint_extruder/footprint_extruder.cpp:143-213;
 *                                           a CPU loop upstream, "the end-to-end bottleneck", README.md:101)
 *   gcv_points_to_volume                   voxlib.points_to_volume
 *                                          (extensions/voxlib/points_to_volume.cu:21-81, bindings.cpp:36)
 *   gcv_maps_to_volume                     voxlib.maps_to_volume
 *                                          (extensions/voxlib/maps_to_volume.cu:21-142, bindings.cpp:38; no in-tree caller)
 *   gcv_ray_voxel_intersection             voxlib.ray_voxel_intersection_perspective
 *                                          (extensions/voxlib/ray_voxel_intersection.cu:54-332, bindings.cpp:33)
 *   gcv_visible_count / gcv_visible_emit   scripts/inference.py:338-341 (_get_bev_points: the visible rows),
 *                                          :345-360 (_get_normalized_pt_cords), :229-237 with :535-598
 *                                          (_instances_to_classes) and utils/helpers.py:197-223 (get_point_scales):
 *                                          numpy / a Python loop over instances upstream (ABI v5)
 *   gcv_model_split_count / _emit          scripts/inference.py:239-253 up to the generator calls (:399-507 with
 *                                          utils/helpers.py:127-133 and :183-194): masks, gathers, a Python loop per model
 *                                          and per visible instance upstream (additive to ABI v5)
 *   gcv_gaussian_points                    utils/helpers.py:226-247 (get_gaussian_points) and the per-key torch.cat of
 *                                          scripts/inference.py:500-501
 *   gcv_frame_finish                       scripts/inference.py:255,264-272 (GaussianBlur through the road mask) and :665-667
 *                                          (the uint8 frame): torchvision + ten torch kernels upstream (additive to ABI v5)
 *   gcv_mean_abs_* / gcv_gan_loss_* / gcv_label_map   core/train.py:285 (masked L1), losses/gan.py:55-97 (GANLoss.loss) and
 *                                          models/discriminator.py:177-189 (_smooth_interp): about forty torch kernels per
 *                                          training iteration upstream (additive to ABI v5)
 *   gcv_train_inputs_count / _emit         core/train.py:207-224 (the slices of pts, instances_to_classes, get_point_scales,
 *                                          get_one_hot, get_projection_uv and get_z's grouping): about 20 + 3 I torch
 *                                          kernels and I + 1 host waits per iteration upstream (additive to ABI v5)
 *   gcv_build_occupancy                    (none upstream: 1 bit per 16x16x16 macro cell; lets the traversal
 *                                           jump across empty macro cells, reproducing the reference walk
 *                                           exactly -- results unchanged)
 *
 * Plain C: device pointers + sizes + a HIP stream, no torch types.  Every function returns 0 on
 * success or a negative gcv_status; gcv_last_error() gives the message (per host thread).
 * All pointers are DEVICE pointers unless the name ends in _host.
 */
#ifndef GCV_H
#define GCV_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCV_ABI_VERSION 5

enum gcv_status {
  GCV_OK = 0,
  GCV_ERR_INVALID_ARGUMENT = -1,
  GCV_ERR_HIP = -2,
  GCV_ERR_UNKNOWN_CLASS = -3, /* a pixel's semantic id has no positive scale (upstream never terminates) */
  GCV_ERR_BUFFER_TOO_SMALL = -4
};

int gcv_abi_version(void);
const char* gcv_last_error(void);

/* segInsMap of footprint_extruder.cpp:90-100,201 (scripts/dataset_generator.py:984-1004) */
typedef struct gcv_seg_ins {
  int16_t bldg_ins_min_id, car_ins_min_id, car_semantic_id, bldg_facade_semantic_id, roof_ins_offset;
} gcv_seg_ins;

/* ---- K15: footprint extruder --------------------------------------------------------------
 * Maps are row-major [height][width]: seg/td/bu int16, pts uint8 (numpy bool).
 * scale_of_semantic: int16[32768], scale_of_semantic[s] = scales[classes[s]] (<= 0: unknown).
 * scratch: gcv_extrude_scratch_bytes(height, width) bytes, carried from _count to _emit.
 * _count enqueues the counting pass, waits for it and stores the number of points (upstream's
 * points.size()) in *n_points_host; _emit writes them in upstream's order (row-major pixels,
 * z ascending) as [n][5] int16 = (x, y, z, scale, instanceID) -- the NPY_UINT16 rows of
 * getNumpyArrayFromVector (:66-84) bit for bit. */
size_t gcv_extrude_scratch_bytes(int32_t height, int32_t width);
int gcv_extrude_count(int32_t include_bottom_points, const int16_t* scale_of_semantic, const gcv_seg_ins* seg_ins_host,
                      int32_t height, int32_t width, const int16_t* seg_map, const int16_t* td_hf,
                      const int16_t* bu_hf, const uint8_t* pts_map, void* scratch, size_t scratch_bytes,
                      int64_t* n_points_host, void* hip_stream);
int gcv_extrude_emit(int32_t include_bottom_points, const int16_t* scale_of_semantic, const gcv_seg_ins* seg_ins_host,
                     int32_t height, int32_t width, const int16_t* seg_map, const int16_t* td_hf,
                     const int16_t* bu_hf, const uint8_t* pts_map, const void* scratch, size_t scratch_bytes,
                     int16_t* points_out, int64_t n_points, void* hip_stream);

/* ---- K13: BEV maps -> instance volume (voxlib.maps_to_volume, extensions/voxlib/maps_to_volume.cu:21-142) ----
 * inst_map/td_hf/bu_hf int16 [height][width], pts_map uint8, scales int8 [n_scales] indexed by semantic class
 * (instance < 10 ? instance : 2, as upstream :16-19,44); volume int16 [height][width][depth] (upstream: depth 504)
 * is zeroed and receives the instance id at every z of a border column (roof = instance + 1).  z outside
 * [0, depth) is skipped (upstream writes out of bounds).  scratch8: 8 device bytes.  Waits for completion. */
int gcv_maps_to_volume(const int16_t* inst_map, const int16_t* td_hf, const int16_t* bu_hf, const uint8_t* pts_map,
                       const int8_t* scales, int32_t n_scales, int32_t height, int32_t width, int32_t depth,
                       int16_t* volume, void* scratch8, void* hip_stream);

/* ---- K14: points -> dense volume ------------------------------------------------------------
 * points [n][3] int16 (x, y, z), pt_ids [n] int32, scales [n][3] int16; volume int32 [h][w][d]
 * (d fastest) is zeroed here (upstream torch::zeros) and every point writes its id into the cube
 * [x,x+sx) x [y,y+sy) x [z,z+sz) clipped to the volume.  Where cubes overlap the HIGHEST id wins
 * (upstream's plain stores race; this is the outcome of a sequential loop in point order).
 * occupancy (nullable): gcv_occupancy_bytes(h, w, d) bytes, filled as by gcv_build_occupancy. */
size_t gcv_occupancy_bytes(int32_t h, int32_t w, int32_t d);
int gcv_points_to_volume(int64_t n_points, const int16_t* points, const int32_t* pt_ids, const int16_t* scales,
                         int32_t h, int32_t w, int32_t d, int32_t* volume, uint32_t* occupancy, void* hip_stream);
int gcv_build_occupancy(const int32_t* volume, int32_t h, int32_t w, int32_t d, uint32_t* occupancy, void* hip_stream);

/* Fused form of scripts/dataset_generator.py:1366-1388 (_get_volume) for rows as the extruder writes them:
 * gcv_points_bounds: per-axis min / max of columns 0..2 of n_points > 0 int16 rows of `row_stride` >= 3 elements
 *   (3: bare points, 5: the extruder's rows; further columns are not read); waits for the result (upstream: six
 *   .item() calls).  scratch: gcv_bounds_scratch_bytes() device bytes, contents irrelevant.
 * gcv_rows_to_volume: rows [n][5] = (x, y, z, scale, instance); voxel id = row index + 1, position =
 *   (x, y, z) - offset in int16 arithmetic, cube of `scale` voxels per side -- what _get_volume + points_to_volume
 *   produce for scales = get_point_scales(rows[:, 3]) (utils/helpers.py:197-222, no special classes).
 *   volume_is_zero != 0: the caller guarantees the h*w*d ints are already 0 (a resident workspace restored by
 *   gcv_rows_erase_volume), so the clear -- the longest stage of a frame -- is skipped.
 * gcv_rows_erase_volume: writes 0 over exactly the cubes gcv_rows_to_volume(rows, offset, ...) wrote. */
size_t gcv_bounds_scratch_bytes(void);
int gcv_points_bounds(int64_t n_points, const int16_t* rows, int32_t row_stride, void* scratch, int32_t min_host[3],
                      int32_t max_host[3], void* hip_stream);
int gcv_rows_to_volume(int64_t n_points, const int16_t* rows, const int32_t offset[3], int32_t h, int32_t w, int32_t d,
                       int32_t* volume, uint32_t* occupancy, int32_t volume_is_zero, void* hip_stream);
int gcv_rows_erase_volume(int64_t n_points, const int16_t* rows, const int32_t offset[3], int32_t h, int32_t w,
                          int32_t d, int32_t* volume, void* hip_stream);

/* ---- K12: perspective ray / voxel traversal -----------------------------------------------------
 * volume int32 [dims0][dims1][dims2] with element strides (any layout torch can hand over);
 * cam_ori/cam_dir/cam_up are HOST float[3] (upstream copies them to the CPU, :256-266);
 * cam_c = (c_row, c_col), img_dims = (rows, cols).  Outputs as upstream (:36-43):
 *   out_voxel_id int32 [rows][cols][max_samples]      0 = no hit
 *   out_depth    float [2][rows][cols][max_samples]   entry t and exit t2; quiet NaN 0x7fc00000 = no hit
 *   out_raydirs  float [rows][cols][3]
 * occupancy (nullable) must describe `volume` with contiguous [h][w][d] strides; it removes steps and
 * memory reads, never changes an output. */
int gcv_ray_voxel_intersection(const int32_t* volume, const int32_t dims[3], const int64_t strides[3],
                               const uint32_t* occupancy, const float cam_ori_host[3], const float cam_dir_host[3],
                               const float cam_up_host[3], float cam_f, const float cam_c[2],
                               const int32_t img_dims[2], int32_t max_samples, int32_t* out_voxel_id,
                               float* out_depth, float* out_raydirs, void* hip_stream);

/* ---- K16: visible point set -> generator inputs (ABI v5) ------------------------------------------
 * What scripts/inference.py does on the host between get_visible_points and the generator, for rows and a
 * first-hit map that are already on the device.  M = number of distinct non-negative values of vp_map.
 *   vp_map   int64 [n_pixels]: row index of the point a pixel sees, any negative value = none
 *            (gcv_ray_voxel_intersection's ids - 1); a value >= n_points is GCV_ERR_INVALID_ARGUMENT, reported by
 *            gcv_visible_count through a device flag, and is never used as an index
 *   rows     int16 [n_points][5] = (x, y, z, scale, instance), as gcv_extrude_emit writes them
 *   centers  float64 [n_centers][5] = (cx, cy, w, h, d); row i belongs to instance id i, cx = NaN marks an
 *            instance that is not in the table (CENTERS.pkl is a dict upstream, :131)
 * Outputs of gcv_visible_emit (all written in full; all but point_index and points8 may be NULL = skipped):
 *   point_index int64 [M]     the distinct non-negative values of vp_map, ascending (:339-340)
 *   points8     float [M][8]  columns 0-4 the int16 row as float; 5-7 the box-relative coordinates of :353-357,
 *                             each evaluated in binary64 in upstream's order and rounded once to binary32:
 *                               rel_x = w > 0 ? (x - cx) / w * 2 : 0,  rel_y likewise with cy, h,
 *                               rel_z = d > 0 ? clip(z / d * 2 - 1, -1, 1) : 0        (16-byte aligned)
 *   instances   int16 [K]     the distinct instance ids of the visible points, ascending (:346)
 *   batch_index int32 [M]     rank of the point's instance in `instances` (:349,358)
 *   classes     float [M]     gcv_class_rule applied to the instance id (:544-598)
 *   scales3     float [M][3]  float(scale) * point_scale_factor (one fp32 multiply) on the three axes, axis 2 = 1
 *                             where the class is in special_z_classes (utils/helpers.py:212-222)
 * A visible point whose instance is negative, >= n_centers or marked NaN is UNKNOWN (KeyError upstream, :351);
 * gcv_visible_count counts them, gcv_visible_emit gives them relative coordinates 0.
 * Count / emit convention of K15: gcv_visible_count enqueues mark + scan, waits, and stores
 * counts_host = {M, K, visible points with an unknown instance}; gcv_visible_emit enqueues and returns.  The
 * workspace (gcv_visible_workspace_bytes, 16-byte aligned) carries the marks from _count to _emit; _count clears
 * what it needs, so one workspace serves frame after frame.  Nothing is allocated inside.  Argument errors (null or
 * misaligned pointers, negative sizes, a small workspace) come back before anything is queued.
 * gcv_visible_workspace_bytes is host only; it returns 0 and sets gcv_last_error() for negative sizes and for
 * n_points or n_pixels >= 2^31. */
typedef struct gcv_class_rule {
  int32_t bldg_ins_min, bldg_ins_max; /* instances in [min, max): facade if even, roof if odd; max <= 0: no upper bound */
  int32_t car_ins_min;                /* instances >= this are cars (applied last, as upstream); <= 0: no cars */
  int32_t facade_class, roof_class, car_class;
  uint32_t special_z_classes;         /* bit c set: class c gets z-scale 1 */
  float point_scale_factor;
} gcv_class_rule;                     /* every other instance keeps its id as its class */
size_t gcv_visible_workspace_bytes(int64_t n_points, int64_t n_pixels);
int gcv_visible_count(const int64_t* vp_map, int64_t n_pixels, const int16_t* rows, int64_t n_points,
                      const double* centers, int32_t n_centers, void* workspace, size_t workspace_bytes,
                      int64_t counts_host[3], void* hip_stream);
int gcv_visible_emit(const int64_t* vp_map, int64_t n_pixels, const int16_t* rows, int64_t n_points,
                     const double* centers, int32_t n_centers, const gcv_class_rule* rule_host, void* workspace,
                     size_t workspace_bytes, int64_t n_visible, int64_t n_instances, int64_t* point_index,
                     float* points8, int32_t* batch_index, int16_t* instances, float* classes, float* scales3,
                     void* hip_stream);

/* ---- K17: visible point set -> per-model generator inputs (additive to ABI v5; probe gcv_model_split_models) ----
 * What scripts/inference.py:239-253 does between the visible set and the generators (_get_pt_indexes_by_models,
 * _get_pt_attrs_by_models, _get_z, utils/helpers.py get_one_hot and get_projection_uv), for K16's outputs as they lie
 * on the device.  A row's model is a function of its class; the per-model batch renumbering and the style groups are
 * prefix counts over K-bit presence tables.
 *   classes float [M], batch_index int32 [M], instances int16 [K], points8 float [M][8], scales3 float [M][3]: K16's outputs
 *   lut_has uint8 [n_lut]: 1 = instance id i has a style code; lut float [n_lut][z_dim]: the codes (n_lut may be 0)
 * gcv_model_rule (HOST): n_classes in [1, 32] (the one-hot's width); model_of_class[c] = 0, 1, 2 for the model slot in
 * upstream's dict order BLDG, CAR, REST, or -1: rows of that class are dropped (upstream skips a model that is None);
 * proj_tlp / proj_size of get_projection_uv (a zero tlp is upstream's `proj_tlp is None` branch bit for bit).
 * gcv_model_split_count enqueues mark + count + scan, waits, and stores
 *   counts_host = {n_0, n_1, n_2,  B_0, B_1, B_2,  G_0, G_1, G_2}: rows per model, distinct instances per model, and how
 *   many of those have a code.  A class that is not an integer in [0, n_classes) or a batch_index outside [0, K) raises a
 *   device flag and is never used as an index: the call returns GCV_ERR_INVALID_ARGUMENT and counts_host is untouched.
 * gcv_model_split_emit enqueues and returns.  A stable three-way partition: rows of model 0 first, in ascending visible-set
 * order (a boolean-mask gather), then model 1, then model 2, in ONE set of buffers of N = n_0 + n_1 + n_2 rows, so a
 * model's tensors are slices.  Outputs (any may be NULL = skipped):
 *   index      int64 [N]             position in the visible set
 *   points8    float [N][8]          the row copied (16-byte aligned, as the input)
 *   batch      int32 [N]             rank of the row's instance among the instances of its own model (:476-480)
 *   classes    float [N], scales3 float [N][3]
 *   onehots    float [N][n_classes]  exactly one 1.0 per row
 *   proj_uv    float [N][2]          ((x - tlp_x) / proj_size) * 2 - 1, likewise y: one rounded fp32 operation each
 *   group      int32 [N]             rank of the row's instance among its model's instances that have a code; -1: it has none
 *   group_instances int16 [G]        G = G_0 + G_1 + G_2: per model (model 0's first) the ids that have a code, ascending
 *   codes      float [G][z_dim]      lut[group_instances[g]]
 * The workspace (gcv_model_split_workspace_bytes(M, K), 16-byte aligned) carries the tables from _count to _emit; _count
 * clears what it needs, so one workspace serves frame after frame.  Nothing is allocated inside; integer atomics only (bit
 * ORs, a counter), so every output is deterministic.  Argument errors (null or misaligned pointers, negative sizes, a small
 * workspace) come back before anything is queued.  gcv_model_split_workspace_bytes is host only; it returns 0 and sets
 * gcv_last_error() for negative sizes, M >= 2^31 and K > 65536. */
typedef struct gcv_model_rule {
  int32_t n_classes;
  int8_t model_of_class[32];
  float proj_tlp[2];
  float proj_size;
} gcv_model_rule;
int gcv_model_split_models(void); /* host only: 3 -- a library that exports it has the entry points of K17 and K18 */
size_t gcv_model_split_workspace_bytes(int64_t n_visible, int64_t n_instances);
int gcv_model_split_count(const float* classes, const int32_t* batch_index, int64_t n_visible, const int16_t* instances,
                          int64_t n_instances, const uint8_t* lut_has, int32_t n_lut, const gcv_model_rule* rule_host,
                          void* workspace, size_t workspace_bytes, int64_t counts_host[9], void* hip_stream);
int gcv_model_split_emit(const float* classes, const int32_t* batch_index, const float* points8, const float* scales3,
                         int64_t n_visible, const int16_t* instances, int64_t n_instances, const uint8_t* lut_has,
                         const float* lut, int32_t n_lut, int32_t z_dim, const gcv_model_rule* rule_host,
                         const void* workspace, size_t workspace_bytes, const int64_t counts_host[9], int64_t* index_out,
                         float* points8_out, int32_t* batch_out, float* classes_out, float* scales3_out, float* onehots_out,
                         float* proj_uv_out, int32_t* group_out, int16_t* group_instances_out, float* codes_out,
                         void* hip_stream);

/* ---- K18: [N][14] Gaussians in one launch (utils/helpers.py:226-247 plus the per-key torch.cat of :500-501) ----
 * out float [n][14] = xyz + dxyz (3), opacity (1), scales * scale (3), rotation (1, 0, 0, 0), rgb (3); one fp32 operation
 * each, opacity 1.0 where the key is absent.  xyz and scales are read with a row stride in elements (K17's points8: 8, its
 * scales3: 3).  Up to three segments (the models, in order) whose rows follow each other: per segment its row count and
 * the generator's outputs rgb [n][3] (required), dxyz [n][3], scale [n][3], opacity [n] -- a key is NULL in every
 * segment that has rows or in none.  The record is HOST memory passed by value.  Inference only; enqueues and returns. */
typedef struct gcv_gaussian_segment {
  int64_t n;
  const float *rgb, *dxyz, *scale, *opacity;
} gcv_gaussian_segment;
typedef struct gcv_gaussian_attrs {
  int32_t n_segments;
  gcv_gaussian_segment seg[3];
} gcv_gaussian_attrs;
int gcv_gaussian_points(const float* xyz, int64_t xyz_stride, const float* scales, int64_t scales_stride, int64_t n,
                 gcv_gaussian_attrs attrs, float* out, void* hip_stream);

/* ---- K19: frame finish -- road-mask blur, composite and the video bytes in one launch (additive to ABI v5; probe
 * gcv_frame_finish_radius_max) ----
 * scripts/inference.py:255,264-272 -- blurrer(img) * road_mask + img * (1 - road_mask) with GaussianBlur's reflect padding
 * -- and the uint8 conversion of :665-667, for a float image and an instance map that are already on the device.
 *   img      float, pixel (b, c, y, x) at img[b * batch_stride + c * channel_stride + y * row_stride + x]: strides in
 *            elements, not negative, pixel stride 1, three channels
 *   ins_map  int16 [height][width] per image, image b's at ins_map + b * map_batch_stride (0: one map for every image)
 *   road     pixel (b, y, x) shows a road where ins_map[b][y][flip_mask_x ? width - 1 - x : x] == road_id
 *   weights_host  HOST float [(2 * radius + 1)^2], row-major; they travel in the kernel's arguments
 * A pixel that shows no road keeps its three floats bit for bit.  A road pixel becomes, per channel,
 *   sum over dy, dx of w[dy][dx] * img[c][refl(y + dy - radius)][refl(x + dx - radius)],   refl(-1) = 1, refl(n) = n - 2
 * (torch's "reflect" padding), in float32, row-major tap order, starting from the first product, one rounding per product
 * and per addition -- a pixel's bits do not depend on how the launch is tiled.
 * Outputs, either or both:
 *   out_f32  float [batch][3][height][width], contiguous; must not overlap the image's extent (not in place)
 *   out_u8   uint8 [batch][height][width][3] = (int)((clamp(v, -1, 1) / 2 + 0.5) * 255) of the value above, a NaN -> 0: the
 *            expression of gcr's out_u8 store; bgr != 0 stores the channels reversed (img[..., ::-1] of :666-667)
 * One launch; does not wait, does not allocate, no atomics, no workspace.  GCV_ERR_INVALID_ARGUMENT before anything is
 * queued for: a null img, ins_map or weights_host; both outputs null; a radius outside 1..gcv_frame_finish_radius_max();
 * a non-positive dimension; height or width <= radius (torch's own condition for reflect padding); a negative stride;
 * batch > 65535; out_f32 overlapping the image.  gcv_frame_finish_radius_max is host only and returns 3. */
int gcv_frame_finish_radius_max(void);
int gcv_frame_finish(const float* img, int64_t batch_stride, int64_t channel_stride, int64_t row_stride, int32_t batch,
                     int32_t height, int32_t width, const int16_t* ins_map, int64_t map_batch_stride, int32_t road_id,
                     int32_t flip_mask_x, int32_t radius, const float* weights_host, float* out_f32, uint8_t* out_u8,
                     int32_t bgr, void* hip_stream);

/* ---- K20-K22: the image losses of a training step (additive to ABI v5; probe gcv_image_loss_max_classes) ----
 * core/train.py:285 (L1Loss()(a * mask, b * mask)), losses/gan.py:55-97 (GANLoss.loss) and
 * models/discriminator.py:177-189 (_smooth_interp), for float tensors that are on the device.  Common to all five:
 *   a tensor is a device pointer and a HOST array of element strides {batch, channel, row} ({batch, row} for a one-channel mask or weight); the
 *   pixel stride is 1, no stride is negative, the element count is below 2^31;
 *   nothing is allocated, nothing waits for the device, there are no atomics; GCV_ERR_INVALID_ARGUMENT before anything is
 *   queued for a null or misaligned pointer, a non-positive size, more than gcv_image_loss_max_classes() classes, a
 *   negative stride, and an output that overlaps an input or another output.
 * A loss is two launches: partial sums per workgroup -- 4096 consecutive elements (K20) or 256 consecutive pixels (K21)
 * each, so the cut depends on the shape alone -- into `partials` (at least gcv_image_loss_partials(n, pixels) doubles,
 * 8-byte aligned, else GCV_ERR_BUFFER_TOO_SMALL), then one workgroup that adds them in a fixed order, divides by the count
 * and stores one float in *loss.  Every addition is binary64, and K21's per-pixel log-sum-exp and softmax are evaluated in
 * binary64 from the float logits: the loss is rounded once.  Two runs give the same bits.  A backward is one launch; it recomputes the terms from the
 * inputs and reads the incoming gradient from the device (grad_loss: one float).
 *
 * K20  loss = sum |t| / (B C H W),  t = fl(fl(a m) - fl(b m)) with mask [B][1][H][W] (any values), a - b with mask NULL
 *      da = fl(fl(g / count) * sign(t)) * m in float, db = -da (sign(0) = 0): contiguous [B][C][H][W], either may be NULL
 * K21  pred [B][C+1][H][W], label [B][C][H][W], weight [B][1][H][W] or NULL; per pixel p_0 := 0, lab_0 := 0,
 *      lse = max + log(sum_c exp(p_c - max)) over c = 0..C;
 *        real != 0: per = sum_{1 <= c < C} lab_c (lse - p_c)        real == 0: per = lse - p_C
 *      loss = mean over B H W of weight * per
 *      dpred contiguous [B][C+1][H][W] = g / count * weight * (softmax_c S - lab_c) (S = sum of the lab_c that count,
 *      lab_C = 0) or (softmax_c - [c == C]); channel 0 is exactly 0.  There is no gradient to label or weight.
 * K22  out contiguous [B][C][h][w], h <= H, w <= W: per output pixel the window rows floor(i H / h) .. ceil((i + 1) H / h) - 1
 *      (columns likewise: adaptive_avg_pool2d's) of seg * mask are summed per channel in row-major order; the channel
 *      with the largest SUM gets 1.0, the others 0.0, a tie goes to the lowest channel (so does an all-zero window).  The
 *      inputs are expected to be finite (torch's argmax prefers a NaN; this comparison does not).  One launch.
 * (K20's entry points are gcv_mean_abs_*: L1Loss is the mean absolute difference, and this library's symbols are letters
 * and underscores only.)
 * gcv_image_loss_max_classes and gcv_image_loss_partials are host only; the latter returns 0 and sets gcv_last_error()
 * for a count outside [1, 2^31). */
int gcv_image_loss_max_classes(void); /* 32 */
int64_t gcv_image_loss_partials(int64_t n_items, int32_t items_are_pixels);
int gcv_mean_abs_forward(const float* a, const int64_t a_strides[3], const float* b, const int64_t b_strides[3], const float* mask,
                   const int64_t mask_strides[2], int32_t batch, int32_t channels, int32_t height, int32_t width,
                   double* partials, int64_t n_partials, float* loss, void* hip_stream);
int gcv_mean_abs_backward(const float* a, const int64_t a_strides[3], const float* b, const int64_t b_strides[3], const float* mask,
                    const int64_t mask_strides[2], int32_t batch, int32_t channels, int32_t height, int32_t width,
                    const float* grad_loss, float* da, float* db, void* hip_stream);
int gcv_gan_loss_forward(const float* pred, const int64_t pred_strides[3], const float* label, const int64_t label_strides[3],
                         const float* weight, const int64_t weight_strides[2], int32_t batch, int32_t classes, int32_t height,
                         int32_t width, int32_t real, double* partials, int64_t n_partials, float* loss, void* hip_stream);
int gcv_gan_loss_backward(const float* pred, const int64_t pred_strides[3], const float* label, const int64_t label_strides[3],
                          const float* weight, const int64_t weight_strides[2], int32_t batch, int32_t classes, int32_t height,
                          int32_t width, int32_t real, const float* grad_loss, float* dpred, void* hip_stream);
int gcv_label_map(const float* seg, const int64_t seg_strides[3], const float* mask, const int64_t mask_strides[2], int32_t batch,
                  int32_t classes, int32_t height, int32_t width, int32_t out_height, int32_t out_width, float* out,
                  void* hip_stream);

/* ---- K23 / K24: the generator's inputs of a training step (additive to ABI v5; probe gcv_train_inputs_max_classes) ----
 * core/train.py:207-224 -- the slices of pts, instances_to_classes (utils/datasets.py:265-282, :333-352), get_point_scales
 * (utils/helpers.py:197-223), get_one_hot (:127-133), get_projection_uv (:183-194) and the grouping of get_z (:136-155) --
 * for the loader's points as they lie on the device.
 *   pts  float rows (x, y, z, scale, instance, rel_x, rel_y, rel_z, batch); row r starts at pts + r * row_stride (elements,
 *        at least 9); n_rows = B * rows_per_batch, batch element b owning rows [b * rows_per_batch, (b + 1) * rows_per_batch)
 * gcv_train_rule (HOST): the dataset's constants.  A row's class is the rule applied to its instance id -- facade for an
 * even id in [bldg_ins_min, bldg_ins_max), roof for an odd one, then car for an id in [car_ins_min, car_ins_max), every
 * other id kept -- the masks taken from the id, never from a class already assigned.
 * Outputs of gcv_train_inputs_emit (any may be NULL = skipped; the columns a skipped output needs are not read):
 *   classes  float [n_rows]             the class
 *   scales3  float [n_rows][3]          scale * scale_factor (one fp32 multiply) three times; axis 2 exactly 1 where the class
 *                                       is an integer c < 32 with bit c of special_z_classes set
 *   onehots  float [n_rows][n_classes]  exactly one 1.0 per row
 *   proj_uv  float [n_rows][2]          ((x - tlp_x) / proj_size) * 2 - 1, likewise y: one rounded fp32 operation each (K17's
 *                                       rule); tlp = proj_tlp[row / rows_per_batch] from DEVICE memory, NULL = upstream's
 *                                       `proj_tlp is None` branch
 *   batch    int64 [n_rows]             (int64) of column 8, truncating
 *   with_groups != 0, after gcv_train_inputs_count on the same rows and workspace:
 *   group    int32 [n_rows]             the rank of the row's instance among the distinct instances, ascending
 *   group_instances int16 [n_instances] those ids; n_instances must be the I that _count stored (it bounds the stores)
 * A row is flagged when its instance is not an integer in [0, 32768) or its class is not an integer in [0, n_classes);
 * it is never used as an index, its one-hot row is all zeros and its group is -1.  gcv_train_inputs_count enqueues a
 * clear, mark and scan, waits, and stores counts_host = {I, rows whose instance is flagged} (it has no rule: a class
 * outside the one-hot is emit's to find).  gcv_train_inputs_emit is one launch and does not wait; its last workgroup
 * stores the number of rows it flagged as a uint32 at byte GCV_TRAIN_INPUTS_FLAG_OFFSET of the workspace, where it stays
 * readable until the next call on that workspace.
 * The workspace (gcv_train_inputs_workspace_bytes(n_rows), 16-byte aligned) holds the 32 768-bit presence table and its
 * word prefix.  _count clears what it uses, so one workspace serves call after call.  An emit with with_groups == 0 needs
 * no count in front of it, on a workspace that was zero-filled once (or has been through a _count): every emit leaves its
 * counters zero again.  Nothing is allocated inside; integer atomics only (bit ORs, counters), so every output is
 * deterministic.  GCV_ERR_INVALID_ARGUMENT before anything is queued for: a null or misaligned pointer (4 bytes; batch 8,
 * group_instances 2, the workspace 16), row_stride < 9, n_rows outside [0, 2^31), n_classes outside 1..32, a proj_size
 * that is zero or no number, a short workspace, rows_per_batch not dividing n_rows, n_instances outside [0, min(n_rows, 32768)].
 * gcv_train_inputs_max_classes and gcv_train_inputs_workspace_bytes are host only; the latter returns 0 and sets
 * gcv_last_error() for n_rows < 0 or >= 2^31. */
#define GCV_TRAIN_INPUTS_FLAG_OFFSET 8
typedef struct gcv_train_rule {
  int32_t bldg_ins_min, bldg_ins_max; /* [min, max): facade if even, roof if odd */
  int32_t car_ins_min, car_ins_max;   /* [min, max): car, applied last as upstream; min >= max: no cars */
  int32_t facade_class, roof_class, car_class;
  int32_t n_classes;          /* 1..32: the one-hot's width */
  uint32_t special_z_classes; /* bit c: class c gets z-scale 1 */
  float scale_factor;         /* cfg.NETWORK.GAUSSIAN.SCALE_FACTOR, one fp32 multiply */
  float proj_size;
} gcv_train_rule;
int gcv_train_inputs_max_classes(void); /* host only: 32 -- a library that exports it has the entry points of K23 and K24 */
size_t gcv_train_inputs_workspace_bytes(int64_t n_rows);
int gcv_train_inputs_count(const float* pts, int64_t row_stride, int64_t n_rows, void* workspace, size_t workspace_bytes,
                           int64_t counts_host[2], void* hip_stream);
int gcv_train_inputs_emit(const float* pts, int64_t row_stride, int64_t n_rows, int64_t rows_per_batch,
                          const gcv_train_rule* rule_host, const float* proj_tlp, void* workspace, size_t workspace_bytes,
                          int32_t with_groups, int64_t n_instances, float* classes, float* scales3, float* onehots,
                          float* proj_uv, int64_t* batch, int32_t* group, int16_t* group_instances, void* hip_stream);

/* avg device ms per stage since the last call (option "timing" of gcv_set_option; hipEvent pairs on the caller's
 * stream, a ring of 8 pairs per stage, so recording never waits for a stage still in flight):
 * 0 extrude_count, 1 extrude_emit, 2 volume_clear, 3 volume_scatter, 4 occupancy, 5 traversal, 6 visible_count,
 * 7 visible_emit */
int gcv_set_option(const char* name, int value);
int gcv_get_stage_ms(float* out, int n);

#ifdef __cplusplus
}
#endif
#endif
