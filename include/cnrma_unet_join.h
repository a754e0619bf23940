/*
 * cnrma_unet_join.h -- C-ABI of libcnrma_unetjoin_hip.so: the decoder joints of the Atlas 3D U-Net
 * (projects/mvsdetection/models/backbone3d.py) on the MI355X (gfx950), one fused pass per decoder level, and the observed mask of
 * the network's input.
 *
 * A library of its own beside libcnrma_unet_hip.so (include/cnrma_unet.h), whose conventions it keeps: every pointer is a DEVICE
 * pointer, buffers are caller-owned and contiguous, the library never allocates, frees, reads the device or synchronises, `stream`
 * is a hipStream_t passed as void*, 0 = ok, negative = -(hipError_t) of a failed launch or CNRMA_UNET_JOIN_EINVAL for bad
 * arguments (answered before any launch); re-entrant, no global mutable state, nothing read from the environment.  Every call is
 * capturable.
 *
 * Reference: projects/mvsdetection/models/backbone3d.py:188-196 (the decoder loop of Backbone3D.forward).
 */
#ifndef CNRMA_UNET_JOIN_H
#define CNRMA_UNET_JOIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_UNET_JOIN_EINVAL (-22)
#define CNRMA_UNET_JOIN_ABI_VERSION 1
/* a magnitude bound is as in cnrma_unet.h (CNRMA_UNET_BOUND_WORDS): 64 slots, one per 64-byte line; the bound is their maximum */
#define CNRMA_UNET_JOIN_BOUND_WORDS 1024

int cnrma_unet_join_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * j1  one decoder joint.  xc [B][Cc][Xc][Yc][Zc] f32 (the decoder state), e [B][Cf][2Xc][2Yc][2Zc] f32 (the encoder skip),
 *     w_up [Cf][Cc] and w_proj [Cf][Cf] f32 (the two bias-free 1x1x1 convolutions, as they lie), scale [Cf], shift [Cf] f32 (the
 *     folded eval-mode BatchNorm; both NULL: no affine map), observed (may be NULL) u8 [B][step 2Xc][step 2Yc][step 2Zc] at the
 *     network's input resolution, out [B][Cf][2Xc][2Yc][2Zc] f32.
 *
 *       u   = w_up . trilinear_x2(xc)            (align_corners = false: along an axis of coarse length n, output index o reads
 *                                                 i0 = floor(max(o / 2 - 0.25, 0)), i1 = min(i0 + 1, n - 1) with weights 1 - l, l,
 *                                                 l = max(o / 2 - 0.25, 0) - i0; indices are clamped by coordinate)
 *       p   = w_proj . e
 *       sel = observed[b][step i][step j][step k] != 0 ? p : u          (sel = p when observed is NULL)
 *       out = (u + max(scale[c] * sel + shift[c], 0)) / 2
 *
 * Arithmetic: exact fp32 on the matrix pipe (32x32x2 fp32 products, fp32 accumulation, channels ascending); w_up is applied on the
 *   coarse grid (the interpolation's weights sum to one, so the two commute) into `scratch`, cnrma_unet_join_scratch_bytes bytes,
 *   16-byte aligned; the eight taps and the epilogue are fp32 in one fixed order.  No atomics on out: the same inputs give the same
 *   bits on every run.
 * bound_out (may be NULL): CNRMA_UNET_JOIN_BOUND_WORDS fp32 words, cleared and written by the call; the maximum of its 64 slots
 *   (words 0, 16, 32, ...) is exactly max|out| over the finite outputs -- what cnrma_unet_conv3_forward takes as bound_x.
 * Cc and Cf multiples of 32 in [32, 256]; B in [1, 65535]; Xc, Yc, Zc >= 1; out below 2^31 elements.
 *
 * cnrma_unet_join_supported: 1 when cnrma_unet_join_forward accepts these sizes, else 0.
 * cnrma_unet_join_scratch_bytes: bytes of `scratch` (0 when unsupported).
 * cnrma_unet_join_forward: three launches (two when bound_out is NULL).  CNRMA_UNET_JOIN_EINVAL, before any launch, for an
 *   unsupported shape, a NULL xc, e, w_up, w_proj, scratch or out, a misaligned scratch, step < 1 with a mask, or a scale without
 *   a shift (or a shift without a scale).
 *
 * j2  cnrma_unet_join_observed: x [B][C][X][Y][Z] f32 -> observed [B][X][Y][Z] u8 = any over c of (x != 0) (so -0.0 is unobserved
 *     and NaN is observed), reading x once; when bound_x != NULL it also receives the magnitude bound of x (its maximum is
 *     max|x| exactly, NaN ignored).  B in [1, 65535], C, X, Y, Z >= 1, x below 2^31 elements.  Two launches (one without bound_x).
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_unet_join_supported(int B, int Cc, int Cf, int Xc, int Yc, int Zc);
size_t cnrma_unet_join_scratch_bytes(int B, int Cc, int Cf, int Xc, int Yc, int Zc);
int cnrma_unet_join_observed(const float* x, int B, int C, int X, int Y, int Z, unsigned char* observed, float* bound_x,
                             void* stream);
int cnrma_unet_join_forward(const float* xc, const float* e, const float* w_up, const float* w_proj, const float* scale,
                            const float* shift, const unsigned char* observed, int step, int B, int Cc, int Cf, int Xc, int Yc,
                            int Zc, void* scratch, float* out, float* bound_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_UNET_JOIN_H */
