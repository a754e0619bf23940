/*
 * cnrma_unet.h -- C-ABI of libcnrma_unet_hip.so: the dense 3x3x3 convolutions of the Atlas 3D U-Net
 * (projects/mvsdetection/models/backbone3d.py) on the MI355X (gfx950), as an implicit GEMM in the project's f16x3 arithmetic.
 *
 * A library of its own beside libcnrma_hip.so (include/cnrma.h), libcnrma_prep_hip.so, libcnrma_eval_hip.so and
 * libcnrma_recon_hip.so.  The conventions are cnrma.h's: every pointer is a DEVICE pointer, buffers are caller-owned and
 * contiguous, the library never allocates, frees, reads the device or synchronises, `stream` is a hipStream_t passed as void*,
 * 0 = ok, negative = -(hipError_t) of a failed launch or CNRMA_UNET_EINVAL for bad arguments (answered before any launch);
 * re-entrant, no global mutable state, nothing read from the environment.  Every call is capturable.
 *
 * Reference: projects/mvsdetection/models/backbone3d.py:73-86 (BasicBlock3d.forward) and :127-201.
 */
#ifndef CNRMA_UNET_H
#define CNRMA_UNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_UNET_EINVAL (-22)
#define CNRMA_UNET_ABI_VERSION 1
/* a magnitude bound is CNRMA_UNET_BOUND_WORDS fp32 words (64 slots, one per 64-byte line); the bound is the maximum of the slots */
#define CNRMA_UNET_BOUND_WORDS 1024

int cnrma_unet_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * u1  y = conv3d(x, w, kernel 3x3x3, padding 1, stride 1 or 2), then the fp32 epilogue.
 *     x [B][Cin][X][Y][Z] f32, y [B][Cout][OX][OY][OZ] f32, both contiguous; OX = (X - 1) / stride + 1 (integer division), OY and
 *     OZ alike.  Cin and Cout multiples of 32 in [32, 256]; B, X, Y, Z >= 1; every tensor below 2^31 elements.
 *
 * Arithmetic (f16x3): x * sx = xh + xm and w * sw = wh + wm with fp16 halves (round to nearest) and power-of-two scales sx, sw
 *   that put the largest magnitude at 2^13..2^14; acc = sum over (tap, cin) of xh wh + xh wm + xm wh on the fp16 matrix pipe with
 *   fp32 accumulation, in one fixed order: cin in chunks of 16 ascending, the 27 taps (dx, dy, dz) ascending, dz fastest, inside a
 *   chunk.  No atomics on y: the same inputs give the same bits on every run.  Taps outside the volume contribute exact zeros.
 * Epilogue, fp32, in this order: v = acc / sx / sw (exact); v = v * scale[c] + shift[c] when scale != NULL (shift then required);
 *   v += residual[same index as y] when residual != NULL; v = max(v, 0) when relu != 0.
 *
 * Magnitude bounds: bound_x and bound_y are CNRMA_UNET_BOUND_WORDS fp32 words each.  bound_x must hold, as the maximum of its
 *   64 slots (words 0, 16, 32, ...), an upper bound of max|x| (cnrma_unet_absmax_f32 writes the exact maximum; a previous
 *   cnrma_unet_conv3_forward's bound_y is one).  bound_y (may be NULL) receives exactly max|y| over the finite outputs: it is
 *   cleared and written by the call, one atomic maximum per workgroup on the slot the workgroup hashes to.
 *
 * cnrma_unet_conv3_supported: 1 when cnrma_unet_conv3_forward accepts these sizes, else 0.
 * cnrma_unet_conv3_weight_bytes: bytes of the prepared weight image (0 for unsupported widths); the image is 16-byte aligned.
 * cnrma_unet_conv3_prepare_weights: w [Cout][Cin][3][3][3] f32 -> image: a 64-byte head {sw, 1 / sw} and the fp16 halves in
 *   matrix-pipe fragment order [Cout / 32][Cin / 16][27 taps][h, m][64 lanes][8].  max|w| is found on the device.  Two launches.
 * cnrma_unet_absmax_f32: bound [CNRMA_UNET_BOUND_WORDS] <- max|x| over n >= 0 elements (NaN ignored).  Two launches.
 * cnrma_unet_conv3_forward: two launches (one when bound_y is NULL).
 * Every call returns CNRMA_UNET_EINVAL for an unsupported shape, a stride other than 1 or 2, a NULL required pointer, a scale
 *   without a shift, or a misaligned image, and launches nothing then.
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_unet_conv3_supported(int B, int Cin, int Cout, int X, int Y, int Z, int stride);
size_t cnrma_unet_conv3_weight_bytes(int Cin, int Cout);
int cnrma_unet_conv3_prepare_weights(const float* w, int Cin, int Cout, void* image, void* stream);
int cnrma_unet_absmax_f32(const float* x, int64_t n, float* bound, void* stream);
int cnrma_unet_conv3_forward(const float* x, const float* bound_x, const void* image, const float* scale, const float* shift,
                             const float* residual, int relu, int stride, int B, int Cin, int Cout, int X, int Y, int Z, float* y,
                             float* bound_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_UNET_H */
