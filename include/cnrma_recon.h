/*
 * cnrma_recon.h -- C-ABI of libcnrma_recon_hip.so: the coarse-to-fine TSDF regression head of the reconstruction half
 * (projects/mvsdetection/models/atlas_head.py) on the MI355X (gfx950): regression, sparsifying fill, loss and backward of ONE scale.
 *
 * A library of its own beside libcnrma_hip.so (include/cnrma.h), libcnrma_prep_hip.so (include/cnrma_prep.h) and
 * libcnrma_eval_hip.so (include/cnrma_eval.h).  The conventions are cnrma.h's: every pointer is a DEVICE pointer, buffers are
 * caller-owned and contiguous, the library never allocates, frees, reads the device or synchronises, `stream` is a hipStream_t
 * passed as void*, 0 = ok, negative = -(hipError_t) of a failed launch or CNRMA_RECON_EINVAL for bad arguments (answered before
 * any launch); re-entrant, no global mutable state, nothing read from the environment.  Every call is capturable.
 *
 * Reference: projects/mvsdetection/models/atlas_head.py:34-86 (AtlasTSDFHead.forward, log_transform).
 */
#ifndef CNRMA_RECON_H
#define CNRMA_RECON_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_RECON_EINVAL (-22)
#define CNRMA_RECON_ABI_VERSION 1

/* element type of the feature volume x (and of dx): the 16-bit codes are cnrma.h's CNRMA_ELEM_F16 / CNRMA_ELEM_BF16 */
#define CNRMA_RECON_ELEM_F32 0
#define CNRMA_RECON_ELEM_F16 1
#define CNRMA_RECON_ELEM_BF16 2

int cnrma_recon_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * r1  One scale of the head.  x [B][C][X][Y][Z] (elem), w [C] f32, tsdf [B][1][X][Y][Z] f32, V = X*Y*Z, B*V < 2^31.
 *     prev [B][1][PX][PY][PZ] f32 is the previous (coarser) scale's output or NULL at the first scale; with prev,
 *     (X, Y, Z) must equal (2 PX, 2 PY, 2 PZ) exactly; without, PX = PY = PZ = 0.
 *
 * cnrma_recon_head_forward: per voxel
 *     u    = prev[b][x >> 1][y >> 1][z >> 1]                        (nearest x2 up-sampling)
 *     near = |u| < threshold          (exactly so: a NaN parent is not near; no prev: every voxel is near)
 *     y    = sum_c x[c] * w[c]        fp32, ascending c, y = fmaf(x[c], w[c], y) from y = 0; 16-bit x widened in registers,
 *                                     so the result equals the fp32 kernel's on the widened volume bit for bit
 *     tsdf = near ? tanhf(y) * label_smoothing : sign(u) * 0.999f   sign(+-0) = sign(NaN) = 0
 *   Voxels that are not near never read x; a wave without a near voxel issues no load of x at all.  One launch.
 *
 * cnrma_recon_head_loss_f32: trgt [B][1][X][Y][Z] f32
 *     use   = (trgt < 1 || all_z(trgt[b][x][y][:] == 1)) && near           (near as above from prev / threshold; NULL prev: true)
 *     lt(v) = sign(v) * log1pf(|v|)
 *     loss  = sum_use |lt(tsdf) - lt(trgt)| / count(use)
 *   Terms in fp32, summed in fp64: per thread in ascending voxel order, lanes by a fixed shuffle tree, waves in order (one partial
 *   per workgroup in `workspace`), the partials by one workgroup in the same fixed way.  No floating-point atomics: the loss is
 *   bit-reproducible.  loss [1] f32 and count [1] i64 stay on the device.  count == 0: loss = NaN at the first scale (NULL prev:
 *   the mean of nothing), exactly 0.0 otherwise.  dloss (may be NULL) [B][1][X][Y][Z] f32 receives d(sum)/d(tsdf) per voxel:
 *   sign(tsdf - trgt) / (1 + |tsdf|) on use voxels with tsdf != 0 (lt is strictly increasing, so this is the sign of
 *   lt(tsdf) - lt(trgt) without its rounding), 0 elsewhere.  Two launches.
 *
 * cnrma_recon_head_backward: g = near ? (grad_tsdf ? grad_tsdf[v] : 0) + (dloss ? grad_loss[0] / count[0] * dloss[v] : 0) : 0
 *   (the loss term is 0 when count[0] == 0), g_y = g * label_smoothing * (1 - (tsdf / label_smoothing)^2), tsdf the saved output;
 *     dx[b][c][v] = g_y[v] * w[c]     written for every voxel (zeros where nothing flows); the fp32 product, rounded once to elem
 *                                     (nearest even): the fp32 kernel's dx converted to elem, bit for bit
 *     dw[c]       = sum_{b,v} g_y[v] * x[b][c][v]       products and sums in fp64: a lane over its 8 voxels in ascending order,
 *                   the lanes of a wave by a fixed shuffle tree (one partial per wave and channel in `workspace`), the partials by
 *                   one workgroup per channel in a fixed order; rounded once to f32.  Voxels with g_y == 0 do not read x.
 *   grad_tsdf, dloss (then grad_loss [1] f32 and count [1] i64 are required), dx and dw may each be NULL.  prev receives no
 *   gradient.  Two launches (one when dw is NULL).
 *
 * cnrma_recon_head_workspace_bytes: bytes of `workspace` (16-byte aligned) that the loss and the backward call of this shape ask
 *   for (the larger of the two; the forward call needs none); 0 for arguments the calls would refuse.
 * Every call returns -22 for B, C, X, Y or Z < 1, B*V >= 2^31, an unknown elem, prev dimensions that are not exactly half of
 *   (X, Y, Z) (or not 0 with a NULL prev), a NULL required pointer or a short workspace.
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_recon_head_workspace_bytes(int B, int C, int X, int Y, int Z);
int cnrma_recon_head_forward(const void* x, int elem, const float* w, const float* prev, int PX, int PY, int PZ, float threshold,
                             float label_smoothing, int B, int C, int X, int Y, int Z, float* tsdf, void* stream);
int cnrma_recon_head_loss_f32(const float* tsdf, const float* prev, int PX, int PY, int PZ, float threshold, const float* trgt,
                              int B, int X, int Y, int Z, void* workspace, size_t workspace_bytes, float* dloss, float* loss,
                              int64_t* count, void* stream);
int cnrma_recon_head_backward(const void* x, int elem, const float* w, const float* prev, int PX, int PY, int PZ, float threshold,
                              float label_smoothing, const float* tsdf, const float* grad_tsdf, const float* dloss,
                              const float* grad_loss, const int64_t* count, int B, int C, int X, int Y, int Z, void* workspace,
                              size_t workspace_bytes, void* dx, float* dw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_RECON_H */
