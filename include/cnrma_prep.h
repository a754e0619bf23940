/*
 * cnrma_prep.h -- C-ABI of libcnrma_prep_hip.so: the data-preparation surface of CN-RMA on the MI355X (gfx950).
 *
 * A library of its own beside libcnrma_hip.so (include/cnrma.h): what prepares ground-truth data before the fusion runs.  The
 * conventions are cnrma.h's: every pointer is a DEVICE pointer, buffers are caller-owned, the library never allocates, frees or
 * synchronises, `stream` is a hipStream_t passed as void*, 0 = ok, negative = -(hipError_t) of a failed launch or
 * CNRMA_PREP_EINVAL for bad arguments; re-entrant, no global mutable state, nothing read from the environment.
 */
#ifndef CNRMA_PREP_H
#define CNRMA_PREP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_PREP_EINVAL (-22)
#define CNRMA_PREP_ABI_VERSION 1

int cnrma_prep_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * p1  Bounds of the fusion volume: order statistics of the back-projected depth pixels   replaces the point cloud and the two
 *     np.quantile calls of data_prepare/scannet/generate_tsdf.py:82-101 (depth_to_world: data_prepare/scannet/tsdf.py:77-101;
 *     data_prepare/arkit/ holds the same lines).  The pinned behaviour is the reference on the CPU, bit for bit.
 * pinv [V][4][4]: inverse of [P[v]; 0 0 0 1], ALL FOUR rows (its last row is not exactly 0 0 0 1; torch.inverse on the host makes
 * it).  depth [V][H][W] row-major.  No point cloud is stored: every pass recomputes the point from its depth pixel.
 * All arithmetic is fp32, un-fused unless written as fma, every division an IEEE division.  For view v, row py, column px:
 *     d   = depth[v][py][px]; d > max_depth -> d = 0                                  (generate_tsdf.py:94; +inf disables it)
 *     p   = ((float)px, (float)py, 1, 1 / d)
 *     Q_r = fma(Pinv[r][3], p3, fma(Pinv[r][2], p2, fma(Pinv[r][1], p1, Pinv[r][0] * p0)))    r = 0..3   (tsdf.py:99 as the CPU's sgemm
 *                                                                                             evaluates it)
 *     w_a = Q_a / Q_3                                                                 a = 0..2   (tsdf.py:100)
 *     kept iff w_0 is finite (generate_tsdf.py:97 tests x only): a depth of 0 or NaN is never kept, a negative depth is.
 *     n = number of kept pixels over all views.
 * Order: the kept w_a of one axis in ascending order s[0 .. n-1], -0.0 counted as +0.0, every NaN last (numpy's sort).
 * Ranks, for q in (q_lo, q_hi) -- as np.quantile (numpy 2) forms them for a float32 sample and a Python-float q, i.e. in fp32:
 *     vi = (float)(n - 1) * (float)q
 *     vi >= (float)(n - 1):  k = k1 = n - 1
 *     otherwise:             k = (int64)floor(vi),  k1 = min((int64)(floor(vi) + 1.0f), n - 1)      (the + 1 is an fp32 sum)
 * out_values [2][3][2] (quantile, axis, (s[k], s[k1])): the EXACT order statistics, found by a radix select over the order-preserving
 *   32-bit key of the float (four passes of 8 bits); the caller interpolates (lo + (hi - lo) * (vi - floor(vi)), numpy's _lerp).
 * out_counts [4] int64: n, and the number of NaNs among the kept values of x, y, z (a NaN makes numpy's quantile of that axis NaN).
 * cnrma_prep_bounds_workspace_bytes: bytes of `workspace` (16-byte aligned; independent of V, H, W; cleared by the call itself).
 * Returns -22, before any launch, for V, H or W < 0, V*H*W >= 2^31, q outside [0, 1] (or NaN), a short or misaligned workspace or a
 *   NULL pointer.  V*H*W == 0 or n == 0 is no error: n = 0 (the NaN counts 0) and out_values is left untouched.
 * Integer atomics only (the sums do not depend on the order), nothing read back, no tuning state.
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_prep_bounds_workspace_bytes(void);
int cnrma_prep_depth_bounds_f32(const float* pinv, const float* depth, int V, int H, int W, float max_depth, double q_lo,
                                double q_hi, void* workspace, size_t workspace_bytes, float* out_values, int64_t* out_counts,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_PREP_H */
