/*
 * cnrma.h -- C-ABI of libcnrma_hip.so: the MI355X (gfx950) hot path of CN-RMA.
 *
 * The reference (SerCharles/CN-RMA) is pure Python over third-party CUDA packages; it has no native ABI of
 * its own.  This header is therefore the boundary a maintainer binds with ctypes: every
 * entry point names the reference Python it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; buffers are caller-owned (torch
 *     allocates them); the library never allocates, frees or synchronises unless stated;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, in order;
 *   - return value: 0 = ok, negative = -(hipError_t) of the failed launch or CNRMA_EINVAL for bad arguments;
 *   - fp32 everywhere the reference is fp32; integer outputs are int32;
 *   - feature maps are consumed channels-last ("NHWC": [V][H][W][C]); cnrma_nchw_to_nhwc_f32 converts the
 *     reference's NCHW layout in one pass;
 *   - re-entrant: no global mutable state.
 */
#ifndef CNRMA_H
#define CNRMA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_EINVAL (-22)
#define CNRMA_ABI_VERSION 7   /* the a13 target / loss entry points (cnrma_fcaf3d_assign_f32, _focal_loss_f32, _positive_losses_f32 and their workspace sizes) are additions inside version 7; 7: + the 16-bit feature-map entry points cnrma_backproject_accum_h16, cnrma_rma_neus_emit_rows_h16, cnrma_rma_emit_features_h16, cnrma_nchw_to_nhwc_b16; no signature changed; 6: the cnrma_debug_* entry points (and the experimental kernels behind them) left the product library: they exist in libcnrma_hip_exp.so (-DCNRMA_EXPERIMENTS) only; no signature changed; 5: + cnrma_sparse_conv_prepare_weights_bf16_t, cnrma_sparse_conv_wgrad_go_bf16, cnrma_sparse_conv_go_bf16 (+ its weight images), cnrma_bn_train_forward_f32 / _backward_f32; 4: gather-once convolution family, records-based point selection (SampleWs layout), *_ref_f32 hand-off */

int cnrma_abi_version(void);

/* A kernel launch that sets n_bytes (a multiple of 4, 4-byte aligned) to `byte` -- unlike a hipMemsetAsync node it re-executes
 * reliably when a captured graph is replayed.  The static trace clears ONE arena per scene with it (all hash tables and
 * neighbour tables of the scene: 0xFF = empty slot / no neighbour) and passes precleared = 1 to the builders below, which
 * then skip their own clearing launch (27 launches per scene). */
int cnrma_fill_bytes_u8(void* dst, int byte, size_t n_bytes, void* stream);

/* out[0] = number of i < n with values[i] < lo[i] or values[i] > hi[i] (n <= 4096).  The static trace registers every capacity /
 * branch assumption of its size plan as such a range on a device word (the live row counts the reference reads back with
 * nonzero() / ME's coordinate manager: ray_marching.py:781, :328-330); this folds them into the scene's status word in ONE launch
 * (it was two compares, an or, a sum and a cast: five). */
int cnrma_range_violations_i32(const int32_t* values, const int32_t* lo, const int32_t* hi, int n, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * layout helper: feat_nchw[V][C][H][W] -> feat_nhwc[V][H][W][C]
 * (the reference keeps NCHW: projects/mvsdetection/models/ray_marching.py:64 and :799 gather [b,:,py,px])
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_nchw_to_nhwc_f32(const float* feat_nchw, float* feat_nhwc, int V, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a1-a3  dense unprojection + accumulate + mean
 * replaces: coordinates()            projects/mvsdetection/datasets/tsdf.py:14-29
 *           backproject()            projects/mvsdetection/models/ray_marching.py:21-69
 *           aggregate_2d_features()  ray_marching.py:220-244   (sum over views, in view order)
 *           clear_3d_features()      ray_marching.py:247-257   (divide by count, zero unseen voxels)
 * proj[V][3][4]: rows 0-1 already divided by backbone2d_stride (ray_marching.py:238-239).
 * volume[C][X][Y][Z] (mean, 0 where count == 0), count[X][Y][Z] int32 (number of views that see the voxel).
 * workspace: NULL, or device memory owned by the caller, 8-byte aligned, one block per call in flight (calls on one stream may
 *   share one).  Two parts:
 *   - the first CNRMA_DENSE_WORKSPACE_BYTES, zeroed once by the caller: only used by the lockstep schedules behind
 *     cnrma_debug_dense_tuning (monotonic arrival counters of their group barriers: never reset; a barrier that timed out or a
 *     change of the group size merely dephases later barriers -- a performance effect, never a correctness one).
 *   - behind them, CNRMA_DENSE_MASK_BYTES(X, Y, Z, V) for the view masks; no clearing needed.  When workspace_bytes >=
 *     CNRMA_DENSE_WORKSPACE_BYTES + CNRMA_DENSE_MASK_BYTES(X, Y, Z, V) and the channels take more than one sweep of the kernel,
 *     the first sweep is launched on its own and records, for every wave, one bit per view: does any of its 64 voxels project
 *     into that view?  The other sweeps (a second launch on the same stream) walk the set bits only (a third of the (wave, view)
 *     pairs at the north-star shape).  The bit is the first sweep's own test, made by the same code on the same lanes from the
 *     same proj on every call (captured graphs included), so volume and count are bit-identical with and without the table.
 *     With less room (NULL, the counters alone, one byte short) one launch walks all V views in every sweep.
 *     cnrma_backproject_accum_h16 uses the workspace in the same way.
 * ---------------------------------------------------------------------------------------------------------- */
#define CNRMA_DENSE_WORKSPACE_BYTES 1024
/* room for the view masks: 8 bytes per wave (64 voxels) and 64 views, for the grid padded to whole bricks (at most 32^3 voxels
 * = 512 waves each) and to a multiple of 8 bricks.  An over-estimate for the shipped 16 x 16 x 32 bricks. */
#define CNRMA_DENSE_MASK_BYTES(X, Y, Z, V)                                                                              \
  ((((((int64_t)(X) + 31) / 32) * (((int64_t)(Y) + 31) / 32) * (((int64_t)(Z) + 31) / 32) + 7) * 512) *               \
   (((int64_t)(V) + 63) / 64) * 8)
int cnrma_backproject_accum_f32(const float* feat_nhwc, const float* proj, int V, int C, int H, int W,
                                int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                float* volume, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream);

/* The same with the feature maps handed over BY REFERENCE: feat_nhwc_ref is a device word holding the address of the
 * channels-last maps (read with one scalar load at kernel start).  A captured launch sequence (HIP graph) bakes its pointer
 * arguments in; through the reference it reads whatever tensor the producer -- the 2D network of ray_marching.py:211-213,
 * run in torch.channels_last -- has just written: the caller stores that tensor's address into the word (an 8-byte copy
 * on the same stream) and replays.  No layout pass, no copy of V x C x H' x W' floats into a static buffer.  C % 4 == 0. */
int cnrma_backproject_accum_ref_f32(const float* const* feat_nhwc_ref, const float* proj, int V, int C, int H, int W,
                                    int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                    float* volume, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream);

/* 16-bit feature maps, read where they lie (the reference runs its 2D stack in half precision under auto_fp16:
 * backbone2d.py:61, fpn.py:150, resnet.py:374; test.py:186-188 wraps the model when a config sets fp16).
 * elem: element type of the maps -- CNRMA_ELEM_F16 (IEEE half) or CNRMA_ELEM_BF16 (bfloat16). */
#define CNRMA_ELEM_F16 1
#define CNRMA_ELEM_BF16 2
/* cnrma_backproject_accum_f32 / _ref_f32 (backproject() ray_marching.py:21-69, aggregate_2d_features() / clear_3d_features()
 * :220-257) on 16-bit channels-last maps: exactly one of feat_nhwc (direct, 16-byte aligned) and feat_nhwc_ref (device word
 * with the maps' address, which must be 16-byte aligned as well) is non-NULL.  C % 8 == 0: a lane gathers 8 channels per
 * 16-byte load.  Both conversions to fp32 are exact and the sum stays fp32 in view order, so volume and count are bit-identical
 * to cnrma_backproject_accum_f32 on the same maps widened to fp32.  CNRMA_EINVAL (nothing is launched) for an unknown elem,
 * both or neither pointer, C % 8 != 0, a misaligned direct pointer, a bad dimension. */
int cnrma_backproject_accum_h16(const void* feat_nhwc, const void* const* feat_nhwc_ref, int elem, const float* proj, int V,
                                int C, int H, int W, int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                float* volume, int32_t* count, void* workspace, int64_t workspace_bytes, void* stream);
/* layout pass for 16-bit elements of either type (bits are moved, never interpreted): feat_nchw[V][C][H][W] -> feat_nhwc[V][H][W][C]
 * (the 2D network's NCHW output, ray_marching.py:211-244, gathered as [b,:,py,px] at :64 and :799) */
int cnrma_nchw_to_nhwc_b16(const void* feat_nchw, void* feat_nhwc, int V, int C, int H, int W, void* stream);

#ifdef CNRMA_EXPERIMENTS
/* libcnrma_hip_exp.so ONLY (built with -DCNRMA_EXPERIMENTS; the product library libcnrma_hip.so exports no cnrma_debug_* symbol
 * and holds no tuning state).  Debug / A-B aid (scripts/dense_ab.py, tests of the alternative voxel orders): overrides the dense
 * kernel's schedule switches {variant, slab, st, zt, tt, zi, chunk, persist, lpv, pipe, epi, lockstep, lattice, nt, own, stagger,
 * groups, ldspad} (host-side global state of that library; n = 0 restores the product configuration). */
int cnrma_debug_dense_tuning(const int* values, int n);
#endif

/* Backward of cnrma_backproject_accum_f32 w.r.t. the feature maps (training):
 * grad_feat_nhwc[v][pix_v(g)][c] += grad_volume[c][g] / count[g] for every valid (voxel g, view v) pair; the output is
 * zeroed first; float atomics (~58 voxels share a pixel), so the sum order is not fixed. */
int cnrma_backproject_backward_f32(const float* grad_volume, const int32_t* count, const float* proj, int V, int C, int H,
                                   int W, int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                   float* grad_feat_nhwc, void* stream);

/* single view, debug/parity: px,py int32 [G] (rounded pixel, INT32_MIN when not finite), valid uint8 [G] */
int cnrma_backproject_index_f32(const float* proj_view, int H, int W, int X, int Y, int Z, float voxel_size,
                                float ox, float oy, float oz, int32_t* px, int32_t* py, uint8_t* valid,
                                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a4  ray parameters      replaces get_ray_parameter()  ray_marching.py:71-111
 * proj_inv[V][4][4] = torch.inverse([P;0 0 0 1]) computed by the host (kept on the host LAPACK so that it is
 * bit-identical to the reference's call at ray_marching.py:100).  o[V][3], d[V][3][H*W].
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_ray_params_f32(const float* proj_inv, int V, int H, int W, float* o, float* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a5/a7  NeuS ray-marching aggregation, two phases (variable-length output)
 * replaces: ray_projection_neus()                 ray_marching.py:687-807
 *           aggregate_2d_features_ray_marching()  ray_marching.py:260-307 (concat of views, w/mean(w) scaling)
 * All V views in one launch; one lane per ray, steps marched in order (fp64 running product like the CPU
 * cumprod at :760).  t_one = sqrt(X^2+Y^2+Z^2)*voxel_size/N as computed in double by the host, rounded to fp32
 * (:710-714).  Sample order everywhere = (view, row, col, step).
 *
 * phase 1  count[V*H*W] int32 kept samples per ray; wsum[V*H*W] fp64 sum of kept weights per ray.
 * then     cnrma_exclusive_scan_i32(count) -> row_offset[V*H*W+1]  (row_offset[last] = M).
 * phase 2  writes rows.  Destination is described by three strided views so that the same kernel serves
 *            (i) the reference's raw rows [M][4+C]      (xyz=rows, w=rows+3, feat=rows+4, all stride 4+C) and
 *            (ii) the fused production layout: coords[Ms][3] (+offset), feats[Ms][C] * (w * inv_mean) with the
 *                 subsample mask of sample_points() applied (fcaf3d_transforms.py:283-296, ray_marching.py:364-405).
 *          sel_index: NULL = every row m goes to output row m; else int32[M], output row of source row m or -1
 *          (an exclusive prefix sum of the keep-mask, -1 where dropped).
 *          w_div: NULL = store features unscaled; else a DEVICE scalar (mean weight, see cnrma_rma_mean_weight):
 *                 features are multiplied by (w / w_div[0]) (:303-304).
 *          out_sample: NULL or int32 [M][2] = (ray index, step) of every row (alignment aid for parity tests).
 *          add[3]: added to xyz (the scene offset of switch_pointcloud, :364); pass zeros for raw rows.
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_rma_neus_count_f32(const float* proj_inv, const float* tsdf, int V, int H, int W, int X, int Y, int Z,
                             float voxel_size, float ox, float oy, float oz, int n_steps, float t_one, float thr,
                             int32_t* count, double* wsum, void* stream);

int cnrma_rma_neus_emit_f32(const float* proj_inv, const float* tsdf, const float* feat_nhwc, int V, int C, int H,
                            int W, int X, int Y, int Z, float voxel_size, float ox, float oy, float oz, int n_steps,
                            float t_one, float thr, const int32_t* row_offset, const int32_t* sel_index,
                            const float* w_div, float addx, float addy, float addz,
                            float* out_xyz, int xyz_stride, float* out_w, int w_stride, float* out_feat,
                            int feat_stride, int32_t* out_sample, void* stream);

/* Single-march variant of the NeuS pair (production path).  cnrma_rma_neus_march_f32 = phase 1 plus a per-ray record
 * of the kept samples: kept[ray][cap] x {int32 weight bits, int32 step} (8 bytes each), cap >= floor(1/thr) + 2 (a
 * ray's weights sum to <= 1, so it keeps at most 1/thr samples; overflow: int32[4] -- [0] counts violations and must read
 * 0, [1..3] are scratch words of the launch).
 * cnrma_rma_neus_emit_rows_f32 = phase 2 from those records: a per-ray pass moves the records of the selected samples to
 * their output position (records: scratch of 16 bytes x n_out), then one 8-lane group per OUTPUT row (n_out of them)
 * writes the row -- nothing is re-marched.
 * Same destination description and arithmetic (place = o + d * (n * t_one)) as cnrma_rma_neus_emit_f32. */
/* sig_table (may be NULL): table[voxel] = sigmoid(-tsdf[voxel]) with the reference's CPU arithmetic, built once per scene by
 * cnrma_rma_sigmoid_table_f32 -- the march then reads it instead of evaluating the sigmoid at every step (same function of
 * the same value: bit-identical weights).  With sig_table == NULL the TSDF is read and the sigmoid evaluated per step. */
int cnrma_rma_sigmoid_table_f32(const float* tsdf, int64_t n, float* table, void* stream);
/* The march's per-scene tables in one call: the sigmoid table and (skip_table != NULL) the free-space skip table -- one byte per
 * 4 x 4 x 4 block of voxels = a radius R = min(4 r, 252) such that every voxel within Chebyshev distance R of any voxel of the
 * block holds the block's table value bit for bit (r: the largest number of blocks such that every block within Chebyshev
 * distance r exists, is a whole block inside the grid and holds the block's value; mixed and partial blocks have 0).  Samples
 * whose successor has the same table value are no-ops of the march (ray_marching.py:759-767: alpha = 0, w = 0 < thr,
 * transmittance x 1), so a ray standing in such a block jumps over the steps that are certain to stay inside the radius without
 * evaluating them: same records, same sums, fewer evaluated steps (rays spend most of their steps in free space).
 * skip_table: cnrma_rma_skip_table_bytes(X, Y, Z) bytes.  Layout, with nb = ceil(X/4) ceil(Y/4) ceil(Z/4) blocks in x-major order
 * and a(n) = n rounded up to a multiple of 256:
 *   [0, nb)                   min(R, 16), one byte per block
 *   [a(nb), a(nb) + 4 nb)     scratch of the build (block values)
 *   [F, F + nb)               R, one byte per block -- what the march reads; F = a(nb) + a(4 nb)
 *   [F + a(nb), F + 3 a(nb))  scratch of the build (two planes of the distance transform) */
size_t cnrma_rma_skip_table_bytes(int X, int Y, int Z);
int cnrma_rma_march_tables_f32(const float* tsdf, int X, int Y, int Z, float* table, void* skip_table, void* stream);
#ifdef CNRMA_EXPERIMENTS
/* libcnrma_hip_exp.so only.  Parity aid: the march's division by the voxel size (reciprocal + two quotient refinements) next to
 * the IEEE division */
int cnrma_debug_div_by_voxel_size_f32(const float* a, int64_t n, float voxel_size, float* q_fast, float* q_ref, void* stream);
#endif
int cnrma_rma_neus_march_f32(const float* proj_inv, const float* tsdf, const float* sig_table, int V, int H, int W, int X,
                             int Y, int Z, float voxel_size, float ox, float oy, float oz, int n_steps, float t_one,
                             float thr, int32_t* count, double* wsum, void* kept, int cap, int32_t* overflow,
                             const void* skip_table, void* stream);       /* skip_table: may be NULL; needs sig_table */

/* The layout pass (cnrma_nchw_to_nhwc_f32) and the march (cnrma_rma_neus_march_f32) of one scene in ONE launch: the two
 * are independent (the march does not read the feature maps), one is a pure HBM stream and the other VALU-bound on
 * cache-resident data, and as separate launches they do not overlap.  Same outputs as the two calls, bit for bit; falls
 * back to two launches when the 16-byte layout kernel does not apply (H*W % 4, C % 4, alignment) or without sig_table. */
int cnrma_nchw_to_nhwc_march_f32(const float* feat_nchw, float* feat_nhwc, int C, const float* proj_inv, const float* tsdf,
                                 const float* sig_table, int V, int H, int W, int X, int Y, int Z, float voxel_size, float ox,
                                 float oy, float oz, int n_steps, float t_one, float thr, int32_t* count, double* wsum,
                                 void* kept, int cap, int32_t* overflow, const void* skip_table, void* stream);

/* Backward of cnrma_rma_neus_emit_rows_f32 w.r.t. the feature maps (training; the weights carry no
 * gradient: the reference computes them under torch.no_grad(), ray_marching.py:705).
 * grad_feat_nhwc[ray][c] = sum over the selected rows j of the ray of grad_out_feat[j][c] * (w_j / w_div[0]); rows are
 * walked in step order from the kept-sample records of the forward march (no atomics; rays without rows get zeros). */
int cnrma_rma_neus_rows_backward_f32(const float* grad_out_feat, int grad_stride, int V, int C, int H, int W,
                                     const int32_t* row_offset, const void* kept, int cap, const int32_t* sel_index,
                                     const float* w_div, float* grad_feat_nhwc, void* stream);
/* n_out = capacity of the output (rows of `records`, grid size); n_out_dev (may be NULL) = device word with the live number of
 * output rows (the n_sel of cnrma_mask_to_index); sel_cap = entries of sel_index (rows >= sel_cap are dropped).
 * kept == NULL and row_offset == NULL: `records` already holds the rows to emit (cnrma_rma_select_records). */
int cnrma_rma_neus_emit_rows_f32(const float* proj_inv, const float* feat_nhwc, int V, int C, int H, int W,
                                 int n_steps, float t_one, const int32_t* row_offset, int64_t n_out,
                                 const int32_t* n_out_dev, const void* kept, int cap, const int32_t* sel_index,
                                 int64_t sel_cap, void* records, const float* w_div, float addx, float addy, float addz,
                                 float* out_xyz, int xyz_stride, float* out_w, int w_stride, float* out_feat,
                                 int feat_stride, int32_t* out_sample, void* stream);
/* ... with the feature maps by reference (see cnrma_backproject_accum_ref_f32) */
int cnrma_rma_neus_emit_rows_ref_f32(const float* proj_inv, const float* const* feat_nhwc_ref, int V, int C, int H, int W,
                                 int n_steps, float t_one, const int32_t* row_offset, int64_t n_out,
                                 const int32_t* n_out_dev, const void* kept, int cap, const int32_t* sel_index,
                                 int64_t sel_cap, void* records, const float* w_div, float addx, float addy, float addz,
                                 float* out_xyz, int xyz_stride, float* out_w, int w_stride, float* out_feat,
                                 int feat_stride, int32_t* out_sample, void* stream);
/* ... with 16-bit feature maps (elem: CNRMA_ELEM_F16 / CNRMA_ELEM_BF16), direct or by reference -- exactly one of the two
 * pointers is non-NULL.  Replaces the gather features[b, :, v, u] * weights of ray_marching.py:289-307, :793-797 for maps the
 * 2D stack wrote in half precision: out_feat = (float)h * (w / w_div[0]), the fp32 expression on the exactly widened element,
 * so every output is bit-identical to cnrma_rma_neus_emit_rows_f32 on the widened maps; outputs stay fp32.  8 channels per
 * 16-byte load where feat_stride % 4 == 0 and out_feat is 16-byte aligned, element by element otherwise.  CNRMA_EINVAL for an
 * unknown elem, both or neither pointer, C % 8 != 0, a direct pointer that is not 16-byte aligned, a bad dimension. */
int cnrma_rma_neus_emit_rows_h16(const float* proj_inv, const void* feat_nhwc, const void* const* feat_nhwc_ref, int elem,
                                 int V, int C, int H, int W,
                                 int n_steps, float t_one, const int32_t* row_offset, int64_t n_out,
                                 const int32_t* n_out_dev, const void* kept, int cap, const int32_t* sel_index,
                                 int64_t sel_cap, void* records, const float* w_div, float addx, float addy, float addz,
                                 float* out_xyz, int xyz_stride, float* out_w, int w_stride, float* out_feat,
                                 int feat_stride, int32_t* out_sample, void* stream);

/* Device-side replacement of sample_points()'s np.random.choice(M, n_keep, replace=False)
 * (fcaf3d_transforms.py:283-296): mask[0..M) gets exactly min(M, n_keep) ones, a uniformly random subset that is a
 * deterministic function of `seed` (smallest n_keep 32-bit hash keys, ties by index).  M = min(m_dev[0], m_cap) is read
 * on the device (no host sync); mask has m_cap entries, those behind M are set to 0.  seed_dev (may be NULL): device word
 * mixed into the seed, so that replays of a captured launch sequence draw fresh subsets.  Same distribution as the
 * reference, different random stream. */
size_t cnrma_sample_workspace_bytes(void);
int cnrma_sample_mask(const int32_t* m_dev, int64_t m_cap, int n_keep, uint32_t seed, const uint32_t* seed_dev,
                      uint8_t* mask, void* workspace, void* stream);
/* sample_points (ray_marching.py:339-358) on the march's per-ray sample records, without the m_cap-sized mask and index:
 * the same random subset as cnrma_sample_mask(m_dev, m_cap, n_keep, seed, seed_dev) -- the keep predicate is a function of
 * the row number -- counted per ray, placed by a scan over the R rays, and written as records[j] = {ray, step, weight bits, 0}
 * in row order (what cnrma_mask_to_index + the record scatter of cnrma_rma_neus_emit_rows_f32 produce); n_sel[0] = rows
 * written (<= min(n_keep, rec_cap)).  row_offset [R + 1] = exclusive scan of the march's counts, kept / cap = its records.
 * Scratch: ray_counts [R], ray_offsets [R + 1], scan_ws cnrma_scan_workspace_bytes(R), sample_ws cnrma_sample_workspace_bytes(). */
int cnrma_rma_select_records(const int32_t* row_offset, int64_t R, const void* kept, int cap, const int32_t* m_dev,
                             int64_t m_cap, int n_keep, uint32_t seed, const uint32_t* seed_dev, void* sample_ws,
                             int32_t* ray_counts, int32_t* ray_offsets, void* scan_ws, int64_t rec_cap, void* records,
                             int32_t* n_sel, void* stream);
/* keep-mask of the k largest scores (ties -> smaller index): the row set of torch.topk(scores, k) as used by the
 * pts_threshold pruning (fcaf3d_head.py:131-137) and nms_pre (:252-256), by 3-pass radix select instead of a sort.
 * n = min(n_dev[0], n_cap) (device); mask has n_cap entries, those behind n are set to 0;
 * workspace: cnrma_sample_workspace_bytes().
 * ORDER: scores are ranked by BIT PATTERN (IEEE total order), not by float comparison: -0.0 ranks below +0.0, a NaN with a
 * clear sign bit ranks above +inf and one with a set sign bit below -inf (torch.topk treats +-0 as equal and every NaN as the
 * largest value); equal bit patterns go by the smaller row. */
int cnrma_topk_mask_f32(const float* scores, const int32_t* n_dev, int64_t n_cap, int k, uint8_t* mask,
                        void* workspace, void* stream);
/* torch.topk(scores, k)[1] for nms_pre (fcaf3d_head.py:252-256), k <= 1024: the same radix select, the kept rows collected
 * in a list and sorted by one workgroup -- out_idx[0..min(n, k)) = rows in descending score order (ties -> smaller row),
 * the slots behind them hold row 0.  k > 1024 returns CNRMA_EINVAL.  workspace: cnrma_sample_workspace_bytes().
 * Same order as cnrma_topk_mask_f32: by bit pattern, so -0.0 comes behind +0.0, a NaN with a clear sign bit first and one with a
 * set sign bit last. */
int cnrma_topk_indices_f32(const float* scores, const int32_t* n_dev, int64_t n_cap, int k, int64_t* out_idx,
                           void* workspace, void* stream);

/* a6  depth variant   replaces ray_projection_depth()  ray_marching.py:809-956
 * Every ray emits exactly NUM = max(1, 2*select_grids) candidate slots; count[ray] = number of slots with
 * weight > 0.  Same two-phase protocol and destination description as the NeuS pair. */
int cnrma_rma_depth_count_f32(const float* proj_inv, const float* tsdf, int V, int H, int W, int X, int Y, int Z,
                              float voxel_size, float ox, float oy, float oz, int n_steps, float t_one,
                              int select_grids, int32_t* count, double* wsum, void* stream);

int cnrma_rma_depth_emit_f32(const float* proj_inv, const float* tsdf, const float* feat_nhwc, int V, int C, int H,
                             int W, int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                             int n_steps, float t_one, int select_grids, const int32_t* row_offset,
                             const int32_t* sel_index, const float* w_div, float addx, float addy, float addz,
                             float* out_xyz, int xyz_stride, float* out_w, int w_stride, float* out_feat,
                             int feat_stride, int64_t sel_cap, int64_t out_cap, void* stream);
/* sel_cap / out_cap (0 = unbounded): capacities of sel_index and of the output buffers when the row count stays on the
 * device (static trace): rows beyond them are dropped instead of written. */

/* Reference quirk: a view whose rays keep exactly ONE sample in total is dropped (ray_marching.py:781-782: squeeze()
 * makes the index 0-dim, len() raises, the bare except skips the view): zeroes that view's counts and weight sums. */
int cnrma_rma_drop_single_sample_views(int32_t* count, double* wsum, int V, int64_t rays_per_view, void* stream);

/* mean_w[0] = (float)(wsum_total[0] / m_total[0])   -- torch.mean(weights), ray_marching.py:303 */
int cnrma_rma_mean_weight(const double* wsum_total, const int32_t* m_total, float* mean_w, void* stream);

/* utilities used between the phases (device-side; no host sync) */
size_t cnrma_scan_workspace_bytes(int64_t n);
/* out[0..n] (n+1 entries): out[i] = sum(in[0..i-1]) */
int cnrma_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* workspace, void* stream);
/* sum of n doubles -> out[0] */
int cnrma_sum_f64(const double* in, double* out, int64_t n, void* workspace, void* stream);
/* mask uint8[n] -> sel_index int32[n] (exclusive rank where mask, -1 elsewhere); total written to n_sel[0] */
int cnrma_mask_to_index(const uint8_t* mask, int32_t* sel_index, int32_t* n_sel, int64_t n, void* workspace,
                        void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a8  switch_pointcloud (test path) on an existing point matrix
 * replaces ray_marching.py:360-405: coord = xyz + offset, keep rows where mask (order preserved).
 * points[M][3+C] -> coords[Ms][3], feats[Ms][C]; sel_index as above (NULL = keep all).
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_select_rows_f32(const float* points, int64_t M, int C, const int32_t* sel_index, float addx, float addy,
                          float addz, float* coords, float* feats, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a9  voxelisation = ME.utils.batch_sparse_collate + ME.SparseTensor(quantization_mode=RANDOM_SUBSAMPLE)
 * replaces ray_marching.py:328-330 (MinkowskiEngine v0.5.4; semantics SURVEY.md Appendix A).
 * q = floor(coord / voxel_size) (true fp32 division) -> int32, batch id prepended; duplicate voxels collapse
 * to the row with the SMALLEST source index (the CPU behaviour of ME).  row_order: 0 = output rows in order of
 * first occurrence; 1 = output rows sorted by the Morton code of (x,y,z) (ME leaves the row order
 * implementation-defined; spatial order makes the convolution gathers cache-friendly and is inherited by every
 * strided level).
 * hash_keys uint64[hash_cap], hash_vals int32[hash_cap]: open-addressing table, hash_cap a power of two >= 2*M;
 * on return it maps voxel key -> output row (reusable as the coordinate map of the level).
 * A coordinate that does not fit the coordinate key (|coord / voxel_size| >= 32767, NaN, batch id >= 65536) makes the call
 * report n_out[0] = -1 (the host raises; the static plan's status word flags it) instead of aliasing another voxel.
 * M = capacity of the input, m_dev (may be NULL) = device word with its live row count.  out_cap (0 = M): rows of the
 * output buffers; unique voxels beyond it are dropped and left unmapped (n_out still counts them: n_out > out_cap tells).
 * out_coords int32[Mu][4] (b,x,y,z), out_feats[Mu][C], out_src int32[Mu], n_out[0] = Mu (device).
 * workspace: cnrma_voxelize_workspace_bytes(M).
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_voxelize_workspace_bytes(int64_t M);
int cnrma_voxelize_f32(const float* coords, const float* feats, int64_t M, const int32_t* m_dev, int C,
                       float voxel_size, int batch_id, int row_order, uint64_t* hash_keys, int32_t* hash_vals,
                       int64_t hash_cap, int32_t* out_coords, float* out_feats, int32_t* out_src, int64_t out_cap,
                       int32_t* n_out, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a10-a11  sparse operators (replace the MinkowskiEngine v0.5.4 surface used by
 *          projects/mvsdetection/models/fcaf3d_backbone.py:26-31,63-70 and fcaf3d_head.py:64-98,107-139,275-298)
 * Coordinates: int32 [N][4] = (batch, x, y, z) at an explicit tensor stride; features fp32 [N][C] row-major.
 * Row counts that are produced on the device are written to int32 device words (n_out) and all kernels that
 * consume such a tensor take BOTH a capacity (grid sizing) and a device pointer to the live row count, so a whole
 * forward can be enqueued without host synchronisation.  Pass n_dev = NULL to use the capacity as the count.
 * ---------------------------------------------------------------------------------------------------------- */

/* coordinate map: build a hash table key(coords[i]) -> i for N unique coordinates */
int cnrma_sparse_build_map(const int32_t* coords, int64_t n_cap, const int32_t* n_dev, uint64_t* hash_keys,
                           int32_t* hash_vals, int64_t hash_cap, int precleared /* hash_keys already hold 0xFF bytes */,
                           void* stream);

/* strided output coordinate set: unique(floor(p / new_stride) * new_stride) in first-occurrence order
 * (MinkowskiConvolution / MinkowskiMaxPooling with stride 2: fcaf3d_backbone.py:26-31, BasicBlock stride 2).
 * Builds the output map (hash) as well.  out_cap (0 = n_cap): rows of out_coords; sites beyond it are dropped and left
 * unmapped (table value -1), n_out still counts them.  workspace: cnrma_voxelize_workspace_bytes(n_cap). */
int cnrma_sparse_stride_coords(const int32_t* in_coords, int64_t n_cap, const int32_t* n_dev, int new_stride,
                               uint64_t* hash_keys, int32_t* hash_vals, int64_t hash_cap, int32_t* out_coords,
                               int64_t out_cap, int32_t* n_out, void* workspace, void* stream);
/* The same set, in the same order, for input rows SORTED by the voxeliser's Morton key (cnrma_voxelize_f32 row_order 1 and every
 * set strided from such a set): the parents' keys are non-decreasing along the rows, so the first row of every parent is found
 * by an adjacent comparison -- no hash table, no atomics.  The coordinate map of the result is not built (cnrma_sparse_build_map
 * when a kernel map needs it).  workspace: cnrma_voxelize_workspace_bytes(n_cap). */
int cnrma_sparse_stride_coords_sorted(const int32_t* in_coords, int64_t n_cap, const int32_t* n_dev, int new_stride,
                                      int32_t* out_coords, int64_t out_cap, int32_t* n_out, void* workspace, void* stream);

/* neighbour table ("kernel map", output-stationary): nbr[No][K] = input row at out_coord + offset[k], or -1.
 * offsets int32 [K][3] in coordinate units (already multiplied by the tensor stride), k with x fastest. */
int cnrma_sparse_kernel_map(const int32_t* out_coords, int64_t no_cap, const int32_t* no_dev,
                            const uint64_t* in_hash_keys, const int32_t* in_hash_vals, int64_t hash_cap,
                            const int32_t* offsets, int K, int32_t* nbr, void* stream);

/* Faster builders of the SAME table for the two structured cases (results identical to cnrma_sparse_kernel_map):
 * _symmetric: stride-1 odd kernel on one coordinate set -- nbr[o][k] = i <=> nbr[i][K-1-k] = o, half the probes;
 * _strided:   stride-2 maps (conv k3 / k1, pooling k2) driven from the input side: an input can only feed the
 *             outputs on the coarse lattice around it (3.4 probes per input for k3, 1 for k2/k1, instead of K per
 *             output); probes go to the OUTPUT set's map.  in_stride = tensor stride of the input. */
int cnrma_sparse_kernel_map_symmetric(const int32_t* coords, int64_t n_cap, const int32_t* n_dev,
                                      const uint64_t* hash_keys, const int32_t* hash_vals, int64_t hash_cap,
                                      const int32_t* offsets, int K, int32_t* nbr, int precleared /* nbr holds 0xFF bytes */,
                                      void* stream);
int cnrma_sparse_kernel_map_strided(const int32_t* in_coords, int64_t n_cap, const int32_t* n_dev, int in_stride,
                                    int kernel_size, const uint64_t* out_hash_keys, const int32_t* out_hash_vals,
                                    int64_t hash_cap, int32_t* nbr, int64_t no_cap, int precleared, void* stream);
/* _children: the 3x3x3 stride-1 table of the set cnrma_sparse_convtr_gen_* generates (fcaf3d_head.py:61-70 up blocks: all 8
 *             children of every parent, child m of parent p at row 8 p + m) from the PARENTS' 3x3x3 table parent_nbr
 *             [np_cap][27]: nbr[8 p + m][k] = 8 * parent_nbr[p][k'] + m' with (k', m') the parent offset / child rank of
 *             child m displaced by offset k -- no hash table, no probes.  nbr [8 * np_cap][27]. */
int cnrma_sparse_kernel_map_children(const int32_t* parent_nbr, int64_t np_cap, const int32_t* np_dev, int32_t* nbr,
                                     void* stream);

/* fused sparse convolution, output-stationary gather-GEMM on fp32 MFMA:
 *   out[o] = act( (sum_k in[nbr[o][k]] @ W[k]) * scale + shift + residual[o] )
 * W[K][Cin][Cout] (ME "kernel" layout), scale/shift per output channel (folded BatchNorm / bias; NULL = 1 / 0),
 * residual [No][Cout] or NULL, act: 0 none, 1 ReLU, 2 ELU(alpha=1).  nbr == NULL means K == 1 identity map.
 * workspace (optional, may be NULL): fp32 scratch for the split over kernel offsets that short layers use to fill
 * the chip (partial slabs reduced in a fixed order: run-to-run deterministic, no atomics);
 * cnrma_sparse_conv_workspace_bytes gives the size that allows the widest split. */
size_t cnrma_sparse_conv_workspace_bytes(int64_t no_cap, int Cout, int K);
int cnrma_sparse_conv_f32(const float* in_feats, int Cin, const int32_t* nbr, int K, const float* weight, int Cout,
                          const float* scale, const float* shift, const float* residual, int act,
                          float* out_feats, int64_t no_cap, const int32_t* no_dev, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Which kernel variant a convolution of these sizes launches (pure host function; the choice depends on the output
 * CAPACITY no_cap, never on live row counts, so a captured launch sequence replays the same kernels): out6 = {tile rows,
 * tile columns, splits over the kernel offsets, offsets per split, load stages in flight (1 | 2), tile shape id}.
 * mode: 0 = fp32 MFMA kernel (cnrma_sparse_conv_f32), 1 = f16x3, 2 = bf16, 3 = bf16x6.  Tests use it to prove which
 * variants a parity case covered (fcaf3d_backbone.py:59-107 / fcaf3d_head.py:61-139 run through all of them). */
int cnrma_sparse_conv_plan(int64_t no_cap, int Cin, int Cout, int K, int mode, int slices, size_t workspace_bytes, int* out6);
#ifdef CNRMA_EXPERIMENTS
/* libcnrma_hip_exp.so ONLY (-DCNRMA_EXPERIMENTS): that library additionally carries the measured-and-rejected kernel forms (the
 * warp-specialised stage kernel, the first and third form of the gather-once convolution, ablation / s_memtime-stamped
 * instantiations); the product library has none of them and no tuning state.
 * Debug / A-B aid (scripts/conv_sweep.py, variant-forcing tests): overrides {tile shape id, splits, load stages in flight,
 * ablation mask} of every later convolution launch (-1 = the launcher's choice; n = 0 restores the product configuration).
 * A non-zero ablation mask routes f16x3 launches to a DIAGNOSTIC kernel that leaves stage components out (timing
 * experiments: its results are meaningless; stage kernel bits: 1 MFMAs, 2 A loads, 4 B loads, 8 LDS stores, 16 barriers;
 * gather-once kernel: 1 MFMAs + fragment reads, 2 union-row loads, 4 weight loads, 8 LDS stores, 16 epilogue stores,
 * 32 local-index load; tile-union builder: 32 / 64 insertion / numbering).  Host-side global state; product code never calls it and nothing reads the
 * environment. */
int cnrma_debug_conv_tuning(const int* values, int n);
#endif

/* fp32-grade convolution on the bf16 matrix cores ("bf16x6": each fp32 operand split exactly into 3 bf16 pieces, the 6
 * significant partial products accumulated in fp32; relative error ~2^-23 per product, i.e. that of an fp32 fma chain;
 * 2.67x fewer matrix-pipe cycles than the fp32 MFMA path).  Needs Cin % 32 == 0.
 * cnrma_sparse_conv_prepare_weights: weight fp32 [K][Cin][Cout] -> weight_split bf16 [3][K][Cin/32][Cout_p][32], Cout_p = Cout
 * rounded up to 128 with zero rows (cnrma_sparse_conv_weight_bytes bytes), done once per layer.  Same arguments /
 * epilogue as cnrma_sparse_conv_f32 otherwise. */
size_t cnrma_sparse_conv_weight_bytes(int K, int Cin, int Cout);
int cnrma_sparse_conv_prepare_weights(const float* weight, int K, int Cin, int Cout, void* weight_split, void* stream);
/* Pre-split feature companions: a feature matrix [N][C] (C % 8 == 0) can carry its bf16 split
 * [N+1][C/8][3 planes][8] (48 bytes per 8 channels; row N is all zeros and stands in for missing neighbours).
 * cnrma_sparse_split_features builds one; the bf16x6 convolutions read it (in_split, may be NULL: then the fp32
 * features are split while they are staged) and write the companion of their OUTPUT in the epilogue (out_split, may be
 * NULL; [no_cap+1] rows), so chains of convolutions never re-split and the gathers carry no VALU work. */
int cnrma_sparse_split_features(const float* feats, int64_t n_cap, const int32_t* n_dev, int C, void* out_split,
                                void* stream);
int cnrma_sparse_conv_bf16x6(const float* in_feats, const void* in_split, int64_t in_zero_row, int Cin,
                             const int32_t* nbr, int K, const void* weight_split, int Cout, const float* scale,
                             const float* shift, const float* residual, int act, float* out_feats, void* out_split,
                             int64_t no_cap, const int32_t* no_dev, void* workspace, size_t workspace_bytes,
                             void* stream);
/* generative transpose (k2 s2) on the same path: weight_split from prepare_weights(K = 8); out_split has 8*n_cap+1 rows */
int cnrma_sparse_convtr_gen_bf16x6(const int32_t* in_coords, const float* in_feats, const void* in_split, int64_t n_cap,
                                   const int32_t* n_dev, int Cin, int half_stride, const void* weight_split, int Cout,
                                   const float* scale, const float* shift, int act, int32_t* out_coords,
                                   float* out_feats, void* out_split, void* stream);

/* Pair-list variant of cnrma_sparse_conv_f16x3 for layers whose kernel map is nearly empty (the stem: a stride-2
 * convolution on a point sample has 1.3-1.5 neighbours per output row, so every row tile of the output-stationary kernel
 * carries all 27 offsets and 95 % of its matrix work multiplies zero rows).  The valid (output, offset) entries of `nbr`
 * are regrouped into a list sorted by offset (runs padded to 128 rows), the MFMA kernel runs over that list with the
 * weight slice chosen per run, and every output row adds its products in ascending offset order (deterministic) before
 * the fused epilogue.  Same operands, same result contract as cnrma_sparse_conv_f16x3 (replaces the same
 * ME.MinkowskiConvolution call: fcaf3d_backbone.py:79-80 of the reference).  pair_cap: capacity of the list, a multiple
 * of 128 and >= (number of valid entries) + 128 * K -- for a stride-2 convolution min(27 * N_out, 8 * N_in) + 128 * K is a
 * provable bound (an input row is a neighbour of at most 2 outputs per axis).  workspace:
 * cnrma_sparse_conv_pairs_workspace_bytes(no_cap, K, Cout, pair_cap) bytes. */
size_t cnrma_sparse_conv_pairs_workspace_bytes(int64_t no_cap, int K, int Cout, int64_t pair_cap);
int cnrma_sparse_conv_pairs_f16x3(const float* in_feats, const float* in_amax, int Cin, const int32_t* nbr, int K,
                                  const void* weight_split, int Cout, const float* scale, const float* shift,
                                  const float* residual, int act, float* out_feats, float* out_amax, int64_t no_cap,
                                  const int32_t* no_dev, int64_t pair_cap, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* The same regrouping in exact fp32 (`v_mfma_f32_32x32x2_f32` over the pair runs; weight = ME layout fp32 [K][Cin][Cout]): the
 * stem of the 256-channel configuration at the reference's own arithmetic (fcaf3d_backbone.py:79-80). */
int cnrma_sparse_conv_pairs_f32(const float* in_feats, int Cin, const int32_t* nbr, int K, const float* weight, int Cout,
                                const float* scale, const float* shift, const float* residual, int act, float* out_feats,
                                int64_t no_cap, const int32_t* no_dev, int64_t pair_cap, void* workspace, size_t workspace_bytes,
                                void* stream);

/* 22-bit convolution on the fp16 matrix cores ("f16x3"): each operand is scaled by a power of two taken from an upper
 * bound of its tensor's magnitude (so that the largest element sits at 2^13..2^14) and split into two fp16 pieces
 * a 2^s = h + m (round to nearest: |a 2^s - h - m| <= 2^-22 |a 2^s|); the products hh + hm + mh are accumulated in fp32 and
 * the scales are removed in the epilogue (exact).  Relative error <= 3 x 2^-22 per product -- below the rounding noise
 * of an fp32 accumulation of the same length -- at half the matrix-pipe cycles and 2/3 of the LDS traffic of bf16x6.
 * Needs Cin % 32 == 0.  A magnitude bound ("amax") is cnrma_amax_bytes() bytes of device memory: 64 words, one per
 * 64-byte line, whose maximum is the bound (blocks publish into the slot their index hashes to: same-address atomics
 * would serialise).  in_amax: bound >= max|in_feats| (cnrma_absmax_f32, or the out_amax of the producing convolution);
 * out_amax (may be NULL): zeroed by the caller, receives max|out_feats|.
 * cnrma_sparse_conv_prepare_weights_f16: weight fp32 [K][Cin][Cout] -> fp16 [2][K][Cin/32][Cout_p][32] of weight * 2^s + a trailer
 * holding max|weight| (cnrma_sparse_conv_f16_weight_bytes bytes in all), done once per layer. */
size_t cnrma_amax_bytes(void);
int cnrma_absmax_f32(const float* in, int64_t n_cap, const int32_t* n_dev, int C, float* out_amax, void* stream);
/* The feature half of cnrma_rma_neus_emit_rows_f32 (ray_marching.py:298-307: point_features * weights / mean(weights)) for point
 * records {ray, step, weight bits, 0} in ANY order: out_feat[j][:] = feat[ray_j][:] * (w_j / w_div[0]), same arithmetic.  The
 * static trace carries the 16-byte records of cnrma_rma_select_records through the voxeliser (as 4-float rows) and emits the
 * features of the surviving representatives straight into the sparse tensor's rows, with their magnitude bound (out_amax:
 * cnrma_amax_bytes() ZEROED bytes, or NULL): no [M, C] intermediate, no row gather, no absmax pass.  Exactly one of feat_nhwc /
 * feat_nhwc_ref (see cnrma_backproject_accum_ref_f32) is given. */
int cnrma_rma_emit_features_f32(const float* feat_nhwc, const float* const* feat_nhwc_ref, int C, const void* records,
                                int64_t n_cap, const int32_t* n_dev, const float* w_div, float* out_feat, int feat_stride,
                                float* out_amax, void* stream);
/* ... with 16-bit feature maps (elem: CNRMA_ELEM_F16 / CNRMA_ELEM_BF16; ray_marching.py:298-307 on maps the 2D stack wrote in half
 * precision): out_feat[j][:] = (float)h * (w_j / w_div[0]), bit-identical to cnrma_rma_emit_features_f32 on the widened maps.  The
 * static trace of a 16-bit slot emits its point features through this one.  C % 8 == 0; a direct pointer is 16-byte aligned. */
int cnrma_rma_emit_features_h16(const void* feat_nhwc, const void* const* feat_nhwc_ref, int elem, int C, const void* records,
                                int64_t n_cap, const int32_t* n_dev, const float* w_div, float* out_feat, int feat_stride,
                                float* out_amax, void* stream);
size_t cnrma_sparse_conv_f16_weight_bytes(int K, int Cin, int Cout);
int cnrma_sparse_conv_prepare_weights_f16(const float* weight, int K, int Cin, int Cout, void* weight_split,
                                          void* stream);
int cnrma_sparse_conv_f16x3(const float* in_feats, const float* in_amax, int Cin, const int32_t* nbr, int K,
                            const void* weight_split, int Cout, const float* scale, const float* shift,
                            const float* residual, int act, float* out_feats, float* out_amax, int64_t no_cap,
                            const int32_t* no_dev, void* workspace, size_t workspace_bytes, void* stream);
/* "Gather-once" form of cnrma_sparse_conv_f16x3 for 3x3x3 stride-1 convolutions (fcaf3d_backbone.py:59-87 BasicBlock
 * convolutions, fcaf3d_head.py:61-83 out / up blocks): same operands, same epilogue, same result up to fp32 rounding order.
 * cnrma_sparse_tile_union_build lists, per 64-row output tile of a neighbour table nbr[no_cap][27], the DISTINCT input rows
 * the tile reads (in groups of kernel offsets whose union fits the LDS image) and the local index of every (row, offset)
 * in that list -- once per (coordinate set, kernel), into cnrma_sparse_tile_union_bytes(no_cap) bytes, reusable by every
 * convolution on that pair.  The convolution then stages a tile's union rows once per 32-channel slice and runs the
 * offsets from LDS without barriers; weights come in MFMA-fragment order (cnrma_sparse_conv_prepare_weights_f16_frag,
 * cnrma_sparse_conv_f16_weight_bytes bytes).  Cin % 32 == 0, Cout >= 64.  workspace: as cnrma_sparse_conv_f32 (slabs of the
 * split over channel slices that short layers use).  tile_counters (may be NULL): ceil(no_cap / 64) * ceil(Cout / 64) zeroed
 * 32-bit words owned by the caller's stream; with them the last block of a tile adds the slabs up itself (same order, same
 * sums as the reduce launch it replaces) and leaves the words zero again.  Measured 2.5-3.5x slower than the reduce launch
 * (device-scope fences per block: an L2 write-back / invalidate each); the plugin passes NULL. */
size_t cnrma_sparse_tile_union_bytes(int64_t no_cap);
int cnrma_sparse_tile_union_build(const int32_t* nbr, int64_t no_cap, const int32_t* no_dev, int K, void* tile_union, void* stream);
int cnrma_sparse_conv_prepare_weights_f16_frag(const float* weight, int K, int Cin, int Cout, void* weight_frag, void* stream);
int cnrma_sparse_conv_go_f16x3(const float* in_feats, const float* in_amax, int Cin, const void* tile_union,
                               const void* weight_frag, int Cout, const float* scale, const float* shift,
                               const float* residual, int act, float* out_feats, float* out_amax, int64_t no_cap,
                               const int32_t* no_dev, void* workspace, size_t workspace_bytes, void* tile_counters,
                               void* stream);
/* What cnrma_sparse_conv_go_f16x3 launches for an output CAPACITY of no_cap rows (a pure host function of the sizes and the
 * workspace: captured launch sequences replay the same kernels; the tests prove variant coverage with it): out8 = {form (1 = the
 * round-5 kernel: metadata requested up front, cached row numbers, scalar offset loop; 0 = the round-4 kernel, kept for the
 * bit-identity test), tile columns (64: the block's four waves are 2 column tiles x 2 offset halves; 128: 4 column tiles),
 * splits over the 32-channel slices (> 1: partial slabs in the workspace + conv_reduce_kernel), slices per split, work order of
 * the one-dimensional grid (0 plain, 1 (column tile, split) groups -> XCDs, 2 row tiles -> XCDs), residual added inside the
 * kernel (0: by the reduce launch), blocks, weight offsets in flight per wave}.  No reference counterpart (ME picks its kernels
 * inside MinkowskiConvolution, fcaf3d_backbone.py:26-31). */
int cnrma_sparse_conv_go_plan(int64_t no_cap, int Cin, int Cout, size_t workspace_bytes, int has_residual, int* out8);
/* Exact-fp32 gather-once convolution (`v_mfma_f32_32x32x2_f32`): the reference's own arithmetic for the 3x3x3 stride-1
 * MinkowskiConvolutions (fcaf3d_backbone.py:26-31, :59-87; fcaf3d_head.py:61-83) on the tile unions of
 * cnrma_sparse_tile_union_build -- same operands / epilogue as cnrma_sparse_conv_f32, an fp32 fma chain per output in the order
 * (32-channel slice, offset group, offset, channel pair).  Weights in MFMA-fragment order, prepared once per layer
 * (cnrma_sparse_conv_prepare_weights_f32_frag into cnrma_sparse_conv_f32_frag_weight_bytes bytes: [K][Cin/32][Cout_p/32][4][64][4]
 * floats).  Cin % 32 == 0, Cout >= 64.  workspace: slabs of the split over channel slices (short layers), as
 * cnrma_sparse_conv_go_f16x3; cnrma_sparse_conv_go_plan describes the launch (the form / in-flight fields do not apply). */
size_t cnrma_sparse_conv_f32_frag_weight_bytes(int K, int Cin, int Cout);
int cnrma_sparse_conv_prepare_weights_f32_frag(const float* weight, int K, int Cin, int Cout, void* weight_frag, void* stream);
int cnrma_sparse_conv_go_f32(const float* in_feats, int Cin, const void* tile_union, const void* weight_frag, int Cout,
                             const float* scale, const float* shift, const float* residual, int act, float* out_feats,
                             int64_t no_cap, const int32_t* no_dev, void* workspace, size_t workspace_bytes, void* stream);
int cnrma_sparse_convtr_gen_f16x3(const int32_t* in_coords, const float* in_feats, const float* in_amax, int64_t n_cap,
                                  const int32_t* n_dev, int Cin, int half_stride, const void* weight_split, int Cout,
                                  const float* scale, const float* shift, int act, int32_t* out_coords,
                                  float* out_feats, float* out_amax, void* stream);

/* bf16 convolution (one bf16 piece per operand, round to nearest, fp32 accumulation: `v_mfma_f32_32x32x16_bf16`) -- the
 * precision of the reference's autocast training configuration (BASELINE configs[4]); NOT within the 1e-4 of the
 * inference path, which stays on f16x3 / f32.  Needs Cin % 32 == 0; weights prepared once:
 * fp32 [K][Cin][Cout] -> bf16 [K][Cin/32][Cout_p][32].  Same arguments / epilogue as cnrma_sparse_conv_f32 otherwise. */
size_t cnrma_sparse_conv_bf16_weight_bytes(int K, int Cin, int Cout);
int cnrma_sparse_conv_prepare_weights_bf16(const float* weight, int K, int Cin, int Cout, void* weight_bf16, void* stream);
/* the image of the data gradient's weights straight from W: Wd[k] = W[flip ? K - 1 - k : k]^T ([Cout] -> [Cin]; needs
 * Cout % 32 == 0; cnrma_sparse_conv_bf16_weight_bytes(K, Cout, Cin) bytes).  flip = 1: for a convolution whose output
 * coordinates ARE its input coordinates (odd kernel, stride 1) the transposed neighbour table is the table with its
 * offsets mirrored, nbr_t[i][k] = nbr[i][K - 1 - k] -- the data gradient runs on the forward table with these weights */
int cnrma_sparse_conv_prepare_weights_bf16_t(const float* weight, int K, int Cin, int Cout, int flip, void* weight_bf16,
                                             void* stream);
int cnrma_sparse_conv_bf16(const float* in_feats, int Cin, const int32_t* nbr, int K, const void* weight_bf16, int Cout,
                           const float* scale, const float* shift, const float* residual, int act, float* out_feats,
                           int64_t no_cap, const int32_t* no_dev, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the sparse convolution (training): what MinkowskiEngine's autograd runs under the reference's
 * train step (ray_marching.py:409-451 forward_train -> fcaf3d_backbone.py:59-107 / fcaf3d_head.py:61-139 convolutions ->
 * loss.backward() in mmcv's optimizer hook) for every ME.MinkowskiConvolution.
 * cnrma_sparse_kernel_map_transpose: nbr_t[n_in][K] with nbr_t[i][k] = o where nbr[o][k] == i (else -1); the data
 *   gradient is then the forward convolution of grad_out over nbr_t with the per-offset transposed weights.
 * cnrma_sparse_conv_wgrad_f32: slabs[chunk][K][Cin][Cout] = sum over the chunk's output rows o of
 *   in_feats[nbr[o][k]]^T (x) grad_out[o] (fp32 MFMA); the weight gradient is the sum of the
 *   cnrma_sparse_conv_wgrad_chunks(no_cap, rows_per_chunk) slabs.  nbr == NULL: identity map (K == 1).
 *   One block of 8 waves per (chunk, offset, 64 x 64 tile), the waves' partial tiles added in a fixed order: every
 *   element of every slab is written (no clearing needed), the result does not depend on scheduling; rows_per_chunk even,
 *   >= 256 keeps all waves busy. */
int cnrma_sparse_kernel_map_transpose(const int32_t* nbr, int64_t no_cap, const int32_t* no_dev, int K, int64_t n_in,
                                      int32_t* nbr_t, void* stream);
int cnrma_sparse_conv_wgrad_chunks(int64_t no_cap, int rows_per_chunk);
int cnrma_sparse_conv_wgrad_f32(const float* in_feats, int Cin, const int32_t* nbr, int K, const float* grad_out, int Cout,
                                int64_t no_cap, const int32_t* no_dev, int rows_per_chunk, float* slabs, void* stream);
/* the same reduction with both operands rounded to bf16 (fp32 accumulation, v_mfma_f32_32x32x16_bf16): the weight
 * gradient of a torch.autocast(bfloat16) training step, as AMP computes it */
int cnrma_sparse_conv_wgrad_bf16(const float* in_feats, int Cin, const int32_t* nbr, int K, const float* grad_out, int Cout,
                                 int64_t no_cap, const int32_t* no_dev, int rows_per_chunk, float* slabs, void* stream);

/* (training, the same ME.MinkowskiConvolution backward; reference configuration: fp16 AMP of configs[4] -> bf16 autocast here)
 * the bf16 weight gradient of a 27-offset convolution on the gather-once structure of its forward
 * (cnrma_sparse_tile_union_build over the same neighbour table): slabs[part][27][Cin][Cout], part = a range of
 * ceil(tiles / parts) 64-row tiles; the weight gradient is the sum of the `parts` slabs, every element of which is written.
 * A block stages a tile's distinct input rows and its grad_out rows once in LDS (bf16, transposed) and runs 7 offsets over
 * them, one per wave; the accumulators live across the part's tiles.  Cin % 4 == Cout % 4 == 0.  Operands rounded to bf16,
 * fp32 accumulation: same products as cnrma_sparse_conv_wgrad_bf16, summed in another (fixed) order. */
int cnrma_sparse_conv_wgrad_go_bf16(const float* in_feats, int Cin, const void* tile_union, const float* grad_out, int Cout,
                                    int64_t no_cap, const int32_t* no_dev, int parts, float* slabs, void* stream);

/* (training: forward and data gradient of the BasicBlock / head 3x3x3 stride-1 ME.MinkowskiConvolution of
 * fcaf3d_backbone.py:59-87 and fcaf3d_head.py:61-83 under autocast)
 * the bf16 convolution (cnrma_sparse_conv_bf16's arithmetic: one bf16 piece per operand, fp32 accumulation) on the
 * gather-once structure of a 27-offset table (cnrma_sparse_tile_union_build): forward and data gradient of the autocast
 * training step.  No epilogue (training composes BatchNorm / activations in torch).  Weight image in MFMA-fragment order:
 *   transpose == 0: W [K][Cin][Cout] as it is (cnrma_sparse_conv_bf16_frag_weight_bytes(K, Cin, Cout) bytes);
 *   transpose == 1: the data gradient's weights W'[k] = W[flip ? K - 1 - k : k]^T (..._weight_bytes(K, Cout, Cin) bytes);
 * the image's input width % 32 == 0, its output width >= 64.  workspace (optional): no_cap x Cout x 4 x (Cin / 32) bytes let
 * short layers split over channel slices. */
size_t cnrma_sparse_conv_bf16_frag_weight_bytes(int K, int Cin, int Cout);
int cnrma_sparse_conv_prepare_weights_bf16_frag(const float* weight, int K, int Cin, int Cout, int transpose, int flip,
                                                void* weight_frag, void* stream);
/* both images of one weight tensor in one launch: the forward's (transpose 0) and the data gradient's (transpose 1, `flip`);
 * Cin % 32 == Cout % 32 == 0 */
int cnrma_sparse_conv_prepare_weights_bf16_frag_pair(const float* weight, int K, int Cin, int Cout, int flip,
                                                     void* frag_forward, void* frag_transposed, void* stream);
int cnrma_sparse_conv_go_bf16(const float* in_feats, int Cin, const void* tile_union, const void* weight_frag, int Cout,
                              float* out_feats, int64_t no_cap, const int32_t* no_dev, void* workspace, size_t workspace_bytes,
                              void* stream);

/* generative transposed convolution k=2 s=2 (fcaf3d_head.py:72-78): 8 children per parent, no overlap.
 * out_coords[8*i+k] = in_coords[i] + {0, half}^3 (k: x fastest); out_feats[8*i+k] = act((in[i] @ W[k])*scale+shift) */
int cnrma_sparse_convtr_gen_f32(const int32_t* in_coords, const float* in_feats, int64_t n_cap, const int32_t* n_dev,
                                int Cin, int half_stride, const float* weight, int Cout, const float* scale,
                                const float* shift, int act, int32_t* out_coords, float* out_feats, void* stream);

/* max pooling over the neighbour table (MinkowskiMaxPooling k=2 s=2, fcaf3d_backbone.py:31) */
int cnrma_sparse_maxpool_f32(const float* in_feats, int C, const int32_t* nbr, int K, float* out_feats,
                             int64_t no_cap, const int32_t* no_dev, void* stream);

/* MinkowskiInstanceNorm of ONE scene's row segment: per-channel mean / biased variance over the rows
 * [row0, row0 + n) -- row0 = *row0_dev (NULL: 0), n = min(n_cap, *n_dev) --, eps = 1e-8, affine (weight, bias),
 * optional ReLU (fcaf3d_backbone.py:29-30).  A multi-scene tensor (scene-major rows) takes one call per scene with the
 * scene's device-side offset / count.  stats_ws: cnrma_instnorm_workspace_bytes(C); on return stats_ws[0..C) = mean,
 * [C..2C) = biased variance (fp64). */
size_t cnrma_instnorm_workspace_bytes(int C);
int cnrma_sparse_instnorm_f32(const float* in_feats, int64_t n_cap, const int32_t* n_dev, const int32_t* row0_dev, int C,
                              const float* weight, const float* bias, float eps, int relu, float* out_feats,
                              double* stats_ws, void* stream);
/* The stem's InstanceNorm - ReLU - MaxPool (fcaf3d_backbone.py:29-31) without the normalised intermediate: out_feats == NULL in
 * cnrma_sparse_instnorm_f32 leaves only the statistics in stats_ws; this entry normalises the candidates of every pooling
 * window on the fly (same operations, same order: bit-identical to the two launches) and publishes max|out| (out_amax:
 * cnrma_amax_bytes() zeroed bytes, or NULL).  C % 4 == 0; nbr [no_cap][K] = the pooling table. */
int cnrma_sparse_instnorm_maxpool_f32(const float* in_feats, int C, const double* stats, const float* weight,
                                      const float* bias, float eps, int relu, const int32_t* nbr, int K, float* out_feats,
                                      int64_t no_cap, const int32_t* no_dev, float* out_amax, void* stream);

/* MinkowskiBatchNorm in training (nn.BatchNorm1d over the rows, fcaf3d_backbone.py / fcaf3d_head.py blocks): the forward is
 * cnrma_sparse_instnorm_f32 with the layer's eps (it leaves {mean, biased variance} in stats_ws); this is the backward:
 * grad_weight = sum dy * xhat, grad_bias = sum dy, grad_in = weight / sigma * (dy - mean(dy) - xhat * mean(dy * xhat)).
 * fp64 column sums in a fixed order (deterministic).  ws: cnrma_instnorm_workspace_bytes(C). */
/* BatchNorm1d in training mode fused with what follows it in a residual block (ME.MinkowskiBatchNorm + MinkowskiReLU of
 * ME's BasicBlock / Bottleneck, reached from fcaf3d_backbone.py:59-107 under the train step):
 *   out = act( (x - mean) / sqrt(var + eps) * weight + bias [+ residual] ),  C <= 256, C % 4 == 0, n >= 2;
 *   act (`relu` / `act`): 0 none, 1 ReLU, 2 ELU (alpha 1: the head's blocks, fcaf3d_head.py:61-83);
 * running_mean / running_var (unbiased estimate) / num_batches_tracked updated in place when given (momentum).
 * stats_ws: cnrma_instnorm_workspace_bytes(C); on return {mean[C], biased variance[C]} in fp64 = the backward's `stats`.
 * backward: y (the forward's output) != NULL applies the activation's derivative to grad_out (ReLU: y > 0; ELU: y + 1 where
 * y <= 0); grad_residual != NULL receives that
 * gradient.  fp64 column sums in a fixed order (deterministic). */
int cnrma_bn_train_forward_f32(const float* x, int64_t n, int C, const float* weight, const float* bias, float eps,
                               const float* residual, int relu, float momentum, float* running_mean, float* running_var,
                               int64_t* num_batches_tracked, float* out, double* stats_ws, void* stream);
int cnrma_bn_train_backward_f32(const float* grad_out, const float* x, const float* y, int act, int64_t n, int C, const double* stats,
                                const float* weight, float eps, float* grad_in, float* grad_residual, float* grad_weight,
                                float* grad_bias, double* ws, void* stream);
int cnrma_bn_backward_f32(const float* grad_out, const float* x, int64_t n, int C, const double* stats, const float* weight,
                          float eps, float* grad_in, float* grad_weight, float* grad_bias, double* ws, void* stream);

/* union-add of two sparse tensors at the same tensor stride (`inputs[i] + x`, fcaf3d_head.py:114):
 * output rows = all rows of A (in order) followed by the rows of B that are not in A.
 * a_hash maps A's coords -> A rows.  out_coords [Na+Nb cap][4], out_feats likewise; n_out device word.
 * On return the A hash additionally maps B-only coords -> their new rows (it becomes the union's map).
 * out_cap (>= na_cap): rows of the output buffers; B-only rows beyond it are dropped (n_out still counts them). */
size_t cnrma_union_workspace_bytes(int64_t nb);
int cnrma_sparse_union_add_f32(const int32_t* a_coords, const float* a_feats, int64_t na_cap, const int32_t* na_dev,
                               const int32_t* b_coords, const float* b_feats, int64_t nb_cap, const int32_t* nb_dev,
                               int C, uint64_t* a_hash_keys, int32_t* a_hash_vals, int64_t hash_cap,
                               int32_t* out_coords, float* out_feats, int64_t out_cap, int32_t* n_out, void* workspace,
                               void* stream);

/* features_at_coordinates (linear interpolation on the coarser lattice, fcaf3d_head.py:129):
 * out[i] = sum over the 8 corners c of floor(q/s)*s + {0,s}^3 of score[c] * prod_d (1 - |q_d - c_d| / s),
 * missing corners contribute 0.  q = query coords (int32 [N][4]), score [Ns][1]. */
int cnrma_sparse_interp_f32(const int32_t* q_coords, int64_t n_cap, const int32_t* n_dev, const float* score,
                            const uint64_t* s_hash_keys, const int32_t* s_hash_vals, int64_t hash_cap,
                            int score_stride, float* out, void* stream);

/* MinkowskiPruning by keep-mask (fcaf3d_head.py:138): rows kept in order. sel_index from cnrma_mask_to_index. */
int cnrma_sparse_prune_f32(const int32_t* in_coords, const float* in_feats, int64_t n_cap, const int32_t* n_dev,
                           int C, const int32_t* sel_index, int32_t* out_coords, float* out_feats, void* stream);

/* row-wise max over channels (scores.features.max(dim=1), fcaf3d_head.py:280) */
int cnrma_rowmax_f32(const float* in, int64_t n_cap, const int32_t* n_dev, int C, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a12  box decoding   replaces FCAF3DHead._bbox_pred_to_bbox  fcaf3d_head.py:300-349 and the score product of
 *      _get_bboxes_single :249  (scores = sigmoid(cls) * sigmoid(centerness)).
 * points int32 coords [n][4] are scaled by voxel_size (:296); reg[n][R] holds exp()'d distances in 0..5 and raw
 * angle terms in 6.. ; yaw_mode: 0 = 6-DoF (R=6), 1 = 'fcaf3d' (R=8 -> 7), 2 = 'sin-cos' (R=8 -> 7), 3 = 'naive' (R=7).
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_fcaf3d_decode_f32(const float* points_xyz, const float* reg, int R, int64_t n, int yaw_mode,
                            float* boxes, void* stream);
/* fused variants used by the production path:
 * head_post: tail of FCAF3DHead.forward_single (fcaf3d_head.py:276-298) over the fused head GEMM output
 *   y[n][ldy] = [centerness | reg(R) | cls(n_cls) | pad] -> centerness[n], bbox_pred[n][R] (exp(scale*reg[:6]), raw
 *   angles), cls[n][n_cls], max_cls[n], points[n][3] = coords[:,1:] * voxel_size; scale = DEVICE scalar (Scale layer).
 * max_score: max_c sigmoid(cls)*sigmoid(centerness), the top-k key of :250-253.
 * select_decode: for the rows ids[0..k) (int64, NULL = identity): scores (:249) and decoded boxes (:300-349). */
int cnrma_fcaf3d_head_post_f32(const float* y, int ldy, const int32_t* coords, int64_t n, int R, int n_cls,
                               const float* scale, float voxel_size, float* centerness, float* bbox_pred, float* cls,
                               float* max_cls, float* points, void* stream);
int cnrma_fcaf3d_max_score_f32(const float* cls, const float* centerness, int64_t n, int n_cls, float* max_score,
                               void* stream);
int cnrma_fcaf3d_select_decode_f32(const int64_t* ids, int64_t k, const float* cls, const float* centerness,
                                   const float* reg, const float* points_xyz, int n_cls, int R, int yaw_mode,
                                   float* scores, float* boxes, void* stream);
int cnrma_fcaf3d_scores_f32(const float* cls, const float* centerness, int64_t n, int n_cls, float* scores,
                            float* max_score, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * "next" row 1: offline 3D NMS   replaces mmdet3d's pcdet_nms_gpu / pcdet_nms_normal_gpu as called by
 * post_process/nms_bbox.py:17-58 (third-party OpenPCDet iou3d_nms semantics: bird's-eye-view IoU, greedy in score order).
 * boxes_sorted [n][7] = (x, y, z, dx, dy, dz, heading), already in descending score order; rotated = 0 ignores heading.
 * mask [n][ceil(n/64)] uint64: bit j of row i set when j > i and IoU(i, j) > iou_thr (the host does the greedy scan).
 * cnrma_box_iou_f32: pairwise IoU matrix [na][nb]; mode3d = 1 multiplies the BEV overlap by the height overlap
 * (the IoU used by the mAP evaluation of post_process/evaluate_bbox.py through mmdet3d's indoor_eval).
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_nms_mask_f32(const float* boxes_sorted, int n, float iou_thr, int rotated, uint64_t* mask, void* stream);
int cnrma_box_iou_f32(const float* a, int na, const float* b, int nb, int rotated, int mode3d, float* iou, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-class 3D NMS of a whole scene on the device   replaces the class loop of post_process/nms_bbox.py:17-58 and the head's
 * own _nms (fcaf3d_head.py:351-392): for every class the rows with score > score_thr, in descending score order (ties: the lower
 * row first), greedy BEV NMS with the suppression test of cnrma_nms_mask_f32 (IoU > iou_thr; box_cols = 7: rotated, 6: axis-aligned).
 * Four launches whatever the data and the class count (rank, mask, scan, gather); no device->host read, no allocation, no
 * synchronisation: capturable in a graph.
 * Input: the padded detection block of the static trace -- boxes [n_cap][box_cols], scores [n_cap][n_cls], n_segments (1..8)
 *   segments of sizes[l] rows (HOST array, sum = n_cap) of which the first valid[l] are live (valid: DEVICE int32 [n_segments],
 *   NULL = every row is live).  Dead rows may hold anything (NaN included) and are never read as candidates.
 *   n_cap <= 4096 (64 lanes x 64 bits: one wave scans a class); anything larger returns CNRMA_EINVAL.
 * Output: out_boxes [out_cap][box_cols], out_scores [out_cap], out_labels int64 [out_cap] -- classes ascending, descending score
 *   inside a class --, n_out[0] = the number of detections (the TRUE total even when it exceeds out_cap; rows from out_cap on
 *   are dropped, rows behind n_out are left as they were).
 * workspace: cnrma_nms_classes_workspace_bytes(n_cap, n_cls) bytes, 16-byte aligned (dominated by the bit masks:
 *   n_cls x n_cap x ceil(n_cap / 64) x 8 bytes; it is not cleared -- the scan reads only words the mask kernel wrote).
 *   The size is 0 for arguments the entry point rejects.
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_nms_classes_workspace_bytes(int n_cap, int n_cls);
int cnrma_nms_classes_f32(const float* boxes, int box_cols, const float* scores, int n_cap, int n_cls, const int32_t* sizes,
                          int n_segments, const int32_t* valid, float score_thr, float iou_thr, void* workspace,
                          size_t workspace_bytes, float* out_boxes, float* out_scores, int64_t* out_labels, int out_cap,
                          int32_t* n_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a13  training targets and detection losses on the device   replaces FCAF3DAssigner.assign / compute_centerness
 *      (fcaf3d_head.py:395-484) and the loss body of FCAF3DHead._loss_single (:172-214: focal loss over all rows, centerness
 *      BCE and IoU3D loss over the positive rows).  No [n, m] plane, no one-hot tensor, no device->host read: each entry point
 *      is a linear chain of launches on `stream`, capturable in a graph, and bit-identical replay to replay.
 * Rows: the levels concatenated -- level_cap[n_levels] (HOST array, n_levels <= 8, sum = n_cap) rows per level, of which the
 *   first level_live[l] are live (DEVICE int32 [n_levels]; NULL = every row is live).  Dead rows may hold anything (NaN
 *   included) and are never read.
 *
 * cnrma_fcaf3d_assign_f32: points [n_cap][3]; boxes [m_cap][7] = (gravity centre, dx, dy, dz, yaw), cs [m_cap][2] =
 *   (cos(-yaw), sin(-yaw)), volume [m_cap], gt_label [m_cap] (int32, or int64 with label_is_i64 = 1), of which the first
 *   m_live[0] (DEVICE word, 0 is legal) are live; 1 <= m_cap <= 1024.  Semantics of FCAF3DAssigner.assign operation for
 *   operation in fp32: inside the box; on the box's best level (first level with fewer than `limit` inside points, minus one,
 *   clamped at 0; the last level if none has fewer); centerness strictly greater than the min(topk + 1, n)-th largest of the
 *   box's column (non-candidates count as -1; a radix select on the float bits, value-exact); then the smallest volume below
 *   1e8, ties to the lowest box index.
 *   Output: labels int32 [n_cap] (-1 on background and dead rows), and the positive rows in ascending row order:
 *   pos_row / pos_box int32 [P_cap], pos_ctr float [P_cap] (the centerness target), n_pos[0] (DEVICE word), with
 *   P_cap = m_cap * topk -- a bound, not a heuristic: condition 3 keeps at most topk rows per box and a row has one box.
 *   Rows of pos_* behind n_pos hold row 0 / box 0 / target 0, so that fixed-shape gathers on them are harmless.
 *   workspace: cnrma_fcaf3d_assign_workspace_bytes(n_cap, n_levels, m_cap) bytes, 16-byte aligned (0 = rejected arguments).
 *
 * cnrma_fcaf3d_focal_loss_f32: cls [n_cap][n_cls] logits, labels int32 [n_cap] (outside [0, n_cls) = background row) ->
 *   loss_sum[0] = the un-normalised sum over live rows and classes of a_t (1 - p_t)^gamma BCE (mmdet FocalLoss,
 *   use_sigmoid=True) and grad_cls [n_cap][n_cls], its derivative (zeros on dead rows).  Partial sums are combined in one
 *   fixed order in fp64.  workspace: cnrma_fcaf3d_focal_loss_workspace_bytes(n_cap, n_cls) bytes, 8-byte aligned.
 *
 * cnrma_fcaf3d_positive_losses_f32: over the p_cap rows of the assignment, of which n_pos[0] are live: logit [p_cap] =
 *   centerness[pos_row], pred_boxes [p_cap][box_cols] = the decoded boxes (cx, cy, cz, dx, dy, dz[, yaw]) of those rows,
 *   boxes [m_cap][7] / pos_box / pos_ctr as above.  sums[0] = sum of BCE-with-logits(logit, pos_ctr), sums[1] = sum of
 *   (1 - IoU3D(pred, boxes[pos_box])) * pos_ctr, sums[2] = sum of pos_ctr; grad_logit [p_cap] and grad_boxes
 *   [p_cap][box_cols] are the derivatives of sums[0] / sums[1] (zeros on dead rows).  rotated = 0: axis-aligned IoU of the
 *   first six columns (box_cols 6 or 7); rotated = 1 (box_cols 7): both boxes rotated about z, the geometry of
 *   core/rotated_iou.py (16 edge crossings + 8 contained corners in angular order, shoelace) with the seven partial
 *   derivatives carried through as forward-mode duals.
 *   workspace: cnrma_fcaf3d_positive_losses_workspace_bytes(p_cap) bytes, 8-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_fcaf3d_assign_workspace_bytes(int64_t n_cap, int n_levels, int m_cap);
int cnrma_fcaf3d_assign_f32(const float* points, const int32_t* level_cap, int n_levels, const int32_t* level_live,
                            const float* boxes, const float* cs, const float* volume, const void* gt_label,
                            int label_is_i64, int m_cap, const int32_t* m_live, int limit, int topk, void* workspace,
                            size_t workspace_bytes, int32_t* labels, int32_t* pos_row, int32_t* pos_box, float* pos_ctr,
                            int32_t* n_pos, void* stream);
size_t cnrma_fcaf3d_focal_loss_workspace_bytes(int64_t n_cap, int n_cls);
int cnrma_fcaf3d_focal_loss_f32(const float* cls, const int32_t* labels, const int32_t* level_cap, int n_levels,
                                const int32_t* level_live, int n_cls, float gamma, float alpha, void* workspace,
                                size_t workspace_bytes, float* loss_sum, float* grad_cls, void* stream);
size_t cnrma_fcaf3d_positive_losses_workspace_bytes(int p_cap);
int cnrma_fcaf3d_positive_losses_f32(const float* logit, const float* pred_boxes, int box_cols, int rotated,
                                     const float* boxes, int m_cap, const int32_t* pos_box, const float* pos_ctr,
                                     const int32_t* n_pos, int p_cap, void* workspace, size_t workspace_bytes, float* sums,
                                     float* grad_logit, float* grad_boxes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a14  mesh of a TSDF volume: marching cubes on the device   replaces TSDF.get_mesh (datasets/tsdf.py:81-114: scikit-image on
 *      the host).  Classic marching cubes with the case table of cnrma_amd/mesh_table.py (csrc/mesh_table.inc): ambiguous faces
 *      are resolved from the face's own four signs, so neighbouring cells agree and the mesh has no cracks.  It is NOT
 *      scikit-image's Lewiner variant triangle for triangle; the edge vertices are the same linear interpolation.
 * tsdf [X][Y][Z] fp32 (z fastest), X*Y*Z <= 2^28.  Field: g = (v == 1) ? 1 : clamp(-v, -1, 1) (tsdf.py:81-114: unobserved
 *   voxels count as inside, level 0); a corner is inside when g > 0 (0 and NaN are outside).  The mesh is EMPTY when no voxel has
 *   g < 0 or none has g > 0 (tsdf.py:81-114: min >= 0 or max <= 0), and when an extent is below 2.
 *
 * cnrma_mesh_workspace_bytes (tsdf.py:81-114): host arithmetic; 0 for arguments the entry points reject.  About 9.1 bytes per
 *   voxel: the compacted list is sized for the worst case, every voxel on it.
 * cnrma_mesh_count_f32 (tsdf.py:81-114): three launches (classify, scan of the block totals, classify + compact) ->
 *   counts[4] (DEVICE) = {n_vertices, n_triangles, n_active_cells, flags}, flags = CNRMA_MESH_HAS_NEGATIVE | CNRMA_MESH_HAS_POSITIVE
 *   as found; the three numbers are 0 for an empty mesh.  workspace: 16-byte aligned, not cleared; it is the input of the emit.
 * cnrma_mesh_emit_f32 (tsdf.py:81-114): one launch over the compacted list -> vertices / normals [v_cap][3] fp32, faces
 *   [f_cap][3] int32.  A vertex is the sign change on an edge owned by its lower voxel: t = g0 / (g0 - g1), position = (voxel
 *   index + t on the edge's axis) * voxel_size + origin3_dev[axis] (un-fused); normal = -(gradient of g interpolated with t between
 *   the edge's ends; central differences * 0.5, one-sided at the border), divided by its length, (0, 0, 0) when that is 0.  Vertex
 *   order: owner (x Y + y) Z + z, then axis; face order: cell index, then table order; faces are counter-clockwise seen from
 *   outside (g <= 0).  Bit-identical from run to run.  Rows at or beyond v_cap / f_cap are never written: a caller whose
 *   capacities are too small sees the true need in counts.  Neither entry point allocates, synchronises or reads the
 *   environment.
 * ---------------------------------------------------------------------------------------------------------- */
#define CNRMA_MESH_HAS_NEGATIVE 1
#define CNRMA_MESH_HAS_POSITIVE 2
size_t cnrma_mesh_workspace_bytes(int X, int Y, int Z);
int cnrma_mesh_count_f32(const float* tsdf, int X, int Y, int Z, void* workspace, size_t workspace_bytes, int32_t* counts,
                         void* stream);
int cnrma_mesh_emit_f32(const float* tsdf, int X, int Y, int Z, float voxel_size, const float* origin3_dev,
                        const void* workspace, float* vertices, float* normals, int64_t v_cap, int32_t* faces, int64_t f_cap,
                        const int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a15  point clouds: voxel down-sample, exact nearest neighbour, metric sums   replaces eval_mesh / nn_correspondance
 *      (post_process/evaluate_mesh.py:29-92: Open3D's voxel_down_sample and a KDTreeFlann queried vertex by vertex from Python).
 * Points are [N][3] fp32, row-major.  Row counts are (n_cap, n_dev): the first min(n_cap, n_dev[0]) rows are live (n_dev DEVICE
 *   word; NULL = n_cap rows); dead rows may hold anything (NaN included) and are never read.  n_cap <= 2^31 - 2.  No entry point
 *   allocates, synchronises or reads the environment; clears are kernel launches; workspaces are 16-byte aligned and their sizes
 *   (host arithmetic, 0 = rejected arguments) are functions of n_cap alone.
 *
 * cnrma_cloud_voxel_downsample_f32: Open3D's voxel_down_sample.  lo[a] = fp32 minimum of coordinate a over the live points;
 *   org[a] = (double)lo[a] - 0.5 * voxel_size; k[a] = floor(((double)p[a] - org[a]) / voxel_size) in fp64 with IEEE division,
 *   un-fused; a voxel is a distinct triple k; its point is (float)(sum of (double)p / count) per axis, the fp64 sum taken in
 *   ascending input index.  Voxels come out in ascending (kx, ky, kz) (Open3D: hash-map order).  out_points [out_cap][3] fp32,
 *   out_count [out_cap] int32 (may be NULL), info[4] (DEVICE) = {number of voxels, flags, 0, 0}.  Rows at or beyond out_cap are
 *   never written; info[0] still holds the true need.  flags: CNRMA_CLOUD_NONFINITE (a live coordinate is NaN or +-inf),
 *   CNRMA_CLOUD_VOXEL_TOO_SMALL (some k[a] >= 2^21: Open3D's "voxel_size is too small"); with a flag up no row is written and
 *   info[0] = 0.  n_cap = 0 (or no live row): 0 voxels, no flags.
 *
 * cnrma_cloud_nn_build_f32: a uniform grid over the live targets in `workspace` (cnrma_cloud_nn_workspace_bytes(n_cap)): the
 *   bounding box, then one thread derives the cell size (`cell`, enlarged by steps of 1.125 until the grid has <= 2^24 cells) and
 *   the dims into a device header; targets sorted by cell (z fastest) as 16-byte records {x, y, z, index} and a CSR of cell
 *   starts.  Targets with a non-finite coordinate, or none at all, give a grid of one cell.
 * cnrma_cloud_nn_query_f32: for every live query q the target t that minimises d2 = (dx*dx + dy*dy) + dz*dz, dx = (double)q.x -
 *   (double)t.x and likewise y, z: fp64, un-fused, in this bracket order; ties go to the lowest target index (the index into the
 *   caller's array).  dist [nq_cap] fp64 = sqrt(d2), idx [nq_cap] int32; no live target: dist = +inf, idx = -1.  Rows behind the
 *   live queries are not written.  The result is a function of the two clouds alone: it does not depend on `cell`, the grid or
 *   the visiting order (shells of cells around the query's cell, until the best is strictly nearer than every unvisited cell can
 *   be).  nt_cap: the n_cap of the build (it places the workspace's parts).  stats (DEVICE uint64 [2], may be NULL; the caller
 *   clears it): += {shells visited, candidates scored} over the live queries -- for measurement, the outputs are the same.
 *
 * cnrma_cloud_score_f64: out3[0] = sum of dist over the live rows (cnrma_sum_f64: one fixed order), out3[1] = number of live
 *   rows with dist < threshold (fp64, strict), out3[2] = number of live rows; all three as fp64 (DEVICE).
 * ---------------------------------------------------------------------------------------------------------- */
#define CNRMA_CLOUD_NONFINITE 1
#define CNRMA_CLOUD_VOXEL_TOO_SMALL 2
size_t cnrma_cloud_downsample_workspace_bytes(int64_t n_cap);
int cnrma_cloud_voxel_downsample_f32(const float* points, int64_t n_cap, const int32_t* n_dev, double voxel_size,
                                     void* workspace, size_t workspace_bytes, float* out_points, int32_t* out_count,
                                     int64_t out_cap, int32_t* info, void* stream);
size_t cnrma_cloud_nn_workspace_bytes(int64_t n_cap);
int cnrma_cloud_nn_build_f32(const float* targets, int64_t n_cap, const int32_t* n_dev, double cell, void* workspace,
                             size_t workspace_bytes, void* stream);
int cnrma_cloud_nn_query_f32(const float* queries, int64_t nq_cap, const int32_t* nq_dev, int64_t nt_cap,
                             const void* workspace, double* dist, int32_t* idx, uint64_t* stats, void* stream);
size_t cnrma_cloud_score_workspace_bytes(int64_t n_cap);
int cnrma_cloud_score_f64(const double* dist, int64_t n_cap, const int32_t* n_dev, double threshold, void* workspace,
                          size_t workspace_bytes, double* out3, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a16  TSDF fusion: posed depth maps into running volumes   replaces TSDFFusion.integrate / get_tsdf
 *      (data_prepare/scannet/tsdf.py:353-474, fed one frame at a time by generate_tsdf.py:104-126; data_prepare/arkit/tsdf.py holds
 *      the same class).  The pinned behaviour is the reference on the CPU, bit for bit, for every voxel.
 * Volumes are flat [N], N = X*Y*Z < 2^31, index (x Y + y) Z + z; images are row-major [H][W], H and W < 2^24.
 *
 * cnrma_tsdf_fuse_f32 (tsdf.py:402-451): integrates views 0 .. V-1 in index order, in place, in ONE launch: a lane owns a voxel and
 *   keeps its six running values in registers across the views, so the volumes are read and written once per launch.
 *   proj [V][12] (row-major 3x4), depth [V][H][W], color [V][3][H][W] or NULL, label [V][H][W] int32 or NULL, origin3_dev [3]:
 *   all DEVICE.  tsdf [N], weight [N], color_vol [3][N] or NULL, label_vol [N] int32 or NULL: DEVICE, in/out (a fresh state is
 *   tsdf 1, weight 0, colour 0, label -1).  All arithmetic is fp32, un-fused unless written as fma:
 *     w_a  = (float)index_a * voxel_size + origin[a]                          (product rounded, then the sum; tsdf.py:376)
 *     cam_r = fma(P[r][3], 1, fma(P[r][2], wz, fma(P[r][1], wy, P[r][0] * wx)))            (tsdf.py:413 as the CPU's sgemm evaluates it)
 *     px = rint(cam_0 / cam_2), py = rint(cam_1 / cam_2) (IEEE division, ties to even), pz = cam_2            (tsdf.py:414-416)
 *     valid = 0 <= px < W and 0 <= py < H and pz > 0, compared as floats (NaN and +-inf fail, -0 passes)              (tsdf.py:420)
 *     d = depth[v][py][px]; d > max_depth -> d = 0 (generate_tsdf.py:119; +inf disables it); valid needs d > 0        (tsdf.py:424)
 *     dist = max((pz - d) / trunc_margin, -1) with a true division (a NaN stays a NaN); valid needs dist < 1     (tsdf.py:427-433)
 *     near = valid and dist > -1                                                                                      (tsdf.py:442)
 *     weight == 0 and valid: tsdf = dist (also when dist == -1: the weight stays 0 and a later view overwrites it again;
 *     tsdf.py:437-438); else near: tsdf += dist (tsdf.py:444-445).  near: weight += 1, color_vol[c] += color[v][c][py][px],
 *     label_vol = label[v][py][px] (the newest wins; tsdf.py:446-451).  weight == 0 is read before the view's own increment.
 *   color / label NULL: that volume is not touched (color_vol / label_vol may then be NULL too).  -22 for a negative size, N >= 2^31,
 *   H or W >= 2^24, color without color_vol, label without label_vol, or a NULL required pointer; V == 0 or N == 0 (or an image
 *   without pixels) is a no-op.  No atomics, no allocation, no synchronisation, nothing read from the environment.
 * cnrma_tsdf_fuse_finish_f32 (tsdf.py:453-474, get_tsdf): tsdf_out[i] = weight[i] > 0 ? tsdf[i] / weight[i] : tsdf[i], and the same
 *   for the three planes of color_vol -> color_out [3][n]; either output may be NULL.  The running volumes are only read.
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_tsdf_fuse_f32(const float* proj, const float* depth, const float* color, const int32_t* label,
                        const float* origin3_dev, int V, int H, int W, int X, int Y, int Z, float voxel_size, float trunc_margin,
                        float max_depth, float* tsdf, float* weight, float* color_vol, int32_t* label_vol, void* stream);
int cnrma_tsdf_fuse_finish_f32(const float* tsdf, const float* weight, const float* color_vol, int64_t n, float* tsdf_out,
                               float* color_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * a17  TSDF resampling: a volume and its attribute volumes under a rigid transform   replaces TSDF.transform
 *      (projects/mvsdetection/datasets/tsdf.py:112-180; with attribute volumes data_prepare/scannet/tsdf.py:266-349: an index grid, a
 *      matrix product, two grid_sample passes and two masked overwrites).  The pinned behaviour is that transform on the CPU, bit for
 *      bit, for every voxel; its matrix product is pinned as the un-fused sum below (the order a BLAS takes is not torch's to choose).
 * src [X][Y][Z] and dst [nx][ny][nz] are DEVICE, row-major (z fastest), each of fewer than 2^31 voxels; X, Y, Z >= 2.
 * src_origin3_dev [3], transform12_dev [3][4] (new world -> old world), dst_origin3_dev [3]: DEVICE.  One lane per output voxel.
 * All arithmetic is fp32, nothing fused, every division an IEEE division.  For output index (i0, i1, i2) and axis a:
 *     w_a = (float)i_a * voxel_size + dst_origin[a]                                     (product rounded, then the sum)
 *     p_r = ((T[r][0] * w_0 + T[r][1] * w_1) + T[r][2] * w_2) + T[r][3] * 1             (un-fused, from the left)
 *     c_a = (p_a - src_origin[a]) / voxel_size
 *     n_a = 2 * c_a / (float)(dim_a - 1) - 1                                            (dim = X, Y, Z)
 *     border = any_a(|n_a| >= 1)                                                        (a NaN compares false)
 *     s_a = ((n_a + 1) * (float)dim_a - 1) / 2          (grid_sample's align_corners=False reading of a grid normalised the
 *                                                        align_corners=True way: kept as the reference has it)
 *     nearest:   index rint(s_a), ties to even; the value is 0 when any index is outside [0, dim_a).  That test stays although
 *                border is tested as well: border voxels of an integer volume without fill are sampled, and s_a may equal
 *                dim_a - 0.5, whose rint is dim_a for an even dim_a.
 *     trilinear: f_a = floor(s_a), lower weight (f_a + 1) - s_a, upper weight s_a - f_a, corner weight (w_z * w_y) * w_x;
 *                acc = +0, then acc += v * weight over the corners INSIDE the volume only, z offset fastest, then y, then x
 *                (ATen's tnw, tne, tsw, tse, bnw, bne, bsw, bse).
 * cnrma_tsdf_resample_f32: near = nearest, lin = trilinear; dst = border ? 1 : (|near| < 1 ? lin : near).  A wave whose voxels are
 *   all on the border stores +1 and reads nothing of src; a wave with no lane in the band |near| < 1 skips the corner gathers.
 * cnrma_tsdf_resample_attr_f32: C channels, src [C][X][Y][Z] -> dst [C][nx][ny][nz], trilinear; no band rule, no border fill
 *   (the reference's rule for float attribute volumes such as 'color').
 * cnrma_tsdf_resample_attr_i64: C channels of int64, nearest; with fill_border != 0 border voxels get border_fill instead (the
 *   reference fills 'semseg' with -1 and leaves 'instance' as sampled, data_prepare/scannet/tsdf.py:327-344).  Labels are gathered
 *   as integers; the reference takes them through fp32, which is the same for |label| < 2^24.
 * Each returns -22, before any launch, for a source dimension below 2, a negative size, a volume of 2^31 voxels or more, or a NULL
 *   pointer; an output without voxels (or C == 0) is a no-op.  No atomics, no reciprocals, no allocation, no synchronisation,
 *   nothing read back, nothing read from the environment.
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_tsdf_resample_f32(const float* src, int X, int Y, int Z, const float* src_origin3_dev, float voxel_size,
                            const float* transform12_dev, const float* dst_origin3_dev, int nx, int ny, int nz, float* dst,
                            void* stream);
int cnrma_tsdf_resample_attr_f32(const float* src, int C, int X, int Y, int Z, const float* src_origin3_dev, float voxel_size,
                                 const float* transform12_dev, const float* dst_origin3_dev, int nx, int ny, int nz, float* dst,
                                 void* stream);
int cnrma_tsdf_resample_attr_i64(const int64_t* src, int C, int X, int Y, int Z, const float* src_origin3_dev, float voxel_size,
                                 const float* transform12_dev, const float* dst_origin3_dev, int nx, int ny, int nz,
                                 int64_t border_fill, int fill_border, int64_t* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_H */
