// TSDF fusion on the device: posed depth maps (and colour / label images) integrated into running volumes (reference:
// data_prepare/scannet/tsdf.py:353-474, TSDFFusion, fed frame by frame by generate_tsdf.py:104-126; about twenty full-volume torch
// passes per frame there).  include/cnrma.h (a16) holds the contract; the pinned behaviour is the reference ON THE CPU, bit for bit.
//
// One lane owns one voxel (flat index (x Y + y) Z + z: a wave owns a z-run) and keeps its tsdf, weight, three colour sums and label in
// registers across the whole view loop: the volumes are read once and written once per launch, however many views it fuses.  The
// projection rows and the origin are wave-uniform (scalar loads).  A wave none of whose voxels falls into a view's image skips that
// view before the gather.  No atomics, no reciprocals, no fused operation that is not an explicit fmaf (the Makefile compiles with
// -ffp-contract=off), nothing read back to the host, no tuning state.
#include <math.h>

#include "common.h"

namespace {

constexpr int FUSION_BLOCK = 256;

struct FusionParams {
  int V, H, W, X, Y, Z;
  float vs, trunc, max_depth;
};

// COLOR: colour images are summed into color_vol; LABEL: label images overwrite label_vol (both pointers non-null then)
template <bool COLOR, bool LABEL>
__global__ __launch_bounds__(FUSION_BLOCK) void fusion_integrate_kernel(FusionParams p, const float* __restrict__ proj,
                                                                        const float* __restrict__ depth,
                                                                        const float* __restrict__ color,
                                                                        const int32_t* __restrict__ label,
                                                                        const float* __restrict__ origin, float* __restrict__ tsdf,
                                                                        float* __restrict__ weight, float* __restrict__ color_vol,
                                                                        int32_t* __restrict__ label_vol) {
  const uint32_t N = (uint32_t)p.X * (uint32_t)p.Y * (uint32_t)p.Z;              // < 2^31 (checked by the entry point)
  const uint32_t g = blockIdx.x * (uint32_t)FUSION_BLOCK + threadIdx.x;
  if (g >= N) return;
  const uint32_t t = g / (uint32_t)p.Z;
  const int z = (int)(g - t * (uint32_t)p.Z), x = (int)(t / (uint32_t)p.Y), y = (int)(t - (uint32_t)x * (uint32_t)p.Y);
  // tsdf.py:376  coords.float() * voxel_size + origin: the product is rounded, then the sum
  const float wx = (float)x * p.vs + origin[0];
  const float wy = (float)y * p.vs + origin[1];
  const float wz = (float)z * p.vs + origin[2];

  float tv = tsdf[g], wv = weight[g];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  int32_t lab = 0;
  if constexpr (COLOR) { c0 = color_vol[g]; c1 = color_vol[(size_t)N + g]; c2 = color_vol[2 * (size_t)N + g]; }
  if constexpr (LABEL) lab = label_vol[g];

  const int64_t hw = (int64_t)p.H * p.W;
  const float fw = (float)p.W, fh = (float)p.H;                                    // exact: H, W < 2^24
  for (int v = 0; v < p.V; ++v) {
    const float* __restrict__ P = proj + (int64_t)v * 12;                         // wave-uniform address
    float cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {                                                 // tsdf.py:413  projection @ world, as the CPU's sgemm
      float acc = P[r * 4 + 0] * wx;                                              // evaluates it (oracle.rma_oracle.matmul_fma_chain)
      acc = fmaf(P[r * 4 + 1], wy, acc);
      acc = fmaf(P[r * 4 + 2], wz, acc);
      acc = fmaf(P[r * 4 + 3], 1.0f, acc);
      cam[r] = acc;
    }
    const float px = rintf(cam[0] / cam[2]), py = rintf(cam[1] / cam[2]), pz = cam[2];        // :414-416  IEEE division, ties to even
    // :420  float comparisons equal the reference's int64 ones: NaN and +-inf convert to INT64_MIN there and fail px >= 0
    bool ok = px >= 0.0f && px < fw && py >= 0.0f && py < fh && pz > 0.0f;
    if (__ballot(ok) == 0ull) continue;                                           // none of the wave's voxels sees this view
    if (!ok) continue;
    const int64_t pix = (int64_t)(int)py * p.W + (int)px;                         // in [0, H W): both tests above passed
    float d = depth[v * hw + pix];
    if (d > p.max_depth) d = 0.0f;                                                // generate_tsdf.py:119
    if (!(d > 0.0f)) continue;                                                    // :424  NaN, zero and negative depths
    const float q = (pz - d) / p.trunc;                                           // :427-428  a true division
    const float dist = q < -1.0f ? -1.0f : q;                                     // torch.clamp(min=-1): a NaN stays a NaN
    if (!(dist < 1.0f)) continue;                                                 // :431
    const bool near = dist > -1.0f;                                               // :442
    if (wv == 0.0f) tv = dist;                                                    // :437-438  also when dist == -1: weight stays 0
    else if (near) tv += dist;                                                    // :444-445
    if (near) {
      wv += 1.0f;                                                                 // :446
      if constexpr (COLOR) {                                                      // :449
        const float* cpix = color + (int64_t)v * 3 * hw + pix;
        c0 += cpix[0];
        c1 += cpix[hw];
        c2 += cpix[2 * hw];
      }
      if constexpr (LABEL) lab = label[v * hw + pix];                             // :451  the newest label wins
    }
  }

  tsdf[g] = tv;
  weight[g] = wv;
  if constexpr (COLOR) { color_vol[g] = c0; color_vol[(size_t)N + g] = c1; color_vol[2 * (size_t)N + g] = c2; }
  if constexpr (LABEL) label_vol[g] = lab;
}

// tsdf.py:461-470  the running sums divided by the weight where it is positive
__global__ __launch_bounds__(FUSION_BLOCK) void fusion_finish_kernel(uint32_t N, const float* __restrict__ tsdf,
                                                                     const float* __restrict__ weight,
                                                                     const float* __restrict__ color_vol, float* __restrict__ tsdf_out,
                                                                     float* __restrict__ color_out) {
  const uint32_t g = blockIdx.x * (uint32_t)FUSION_BLOCK + threadIdx.x;
  if (g >= N) return;
  const float w = weight[g];
  const bool seen = w > 0.0f;
  if (tsdf_out != nullptr) {
    const float t = tsdf[g];
    tsdf_out[g] = seen ? t / w : t;
  }
  if (color_out != nullptr) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float s = color_vol[c * (size_t)N + g];
      color_out[c * (size_t)N + g] = seen ? s / w : s;
    }
  }
}

}  // namespace

extern "C" int cnrma_tsdf_fuse_f32(const float* proj, const float* depth, const float* color, const int32_t* label,
                                   const float* origin3_dev, int V, int H, int W, int X, int Y, int Z, float voxel_size,
                                   float trunc_margin, float max_depth, float* tsdf, float* weight, float* color_vol,
                                   int32_t* label_vol, void* stream) {
  if (V < 0 || H < 0 || W < 0 || X < 0 || Y < 0 || Z < 0) return -22;
  if (H >= (1 << 24) || W >= (1 << 24)) return -22;                 // pixel coordinates are compared as fp32
  const int64_t N = (int64_t)X * Y * Z;
  if (N >= ((int64_t)1 << 31)) return -22;
  if ((color != nullptr && color_vol == nullptr) || (label != nullptr && label_vol == nullptr)) return -22;
  if (V == 0 || N == 0 || H == 0 || W == 0) return 0;               // an image without pixels is seen by no voxel
  if (proj == nullptr || depth == nullptr || origin3_dev == nullptr || tsdf == nullptr || weight == nullptr) return -22;
  const FusionParams p{V, H, W, X, Y, Z, voxel_size, trunc_margin, max_depth};
  const dim3 grid((unsigned)ceil_div(N, FUSION_BLOCK)), block(FUSION_BLOCK);
  hipStream_t st = as_stream(stream);
  const bool c = color != nullptr, l = label != nullptr;
  if (c && l) hipLaunchKernelGGL((fusion_integrate_kernel<true, true>), grid, block, 0, st, p, proj, depth, color, label, origin3_dev, tsdf, weight, color_vol, label_vol);
  else if (c) hipLaunchKernelGGL((fusion_integrate_kernel<true, false>), grid, block, 0, st, p, proj, depth, color, label, origin3_dev, tsdf, weight, color_vol, label_vol);
  else if (l) hipLaunchKernelGGL((fusion_integrate_kernel<false, true>), grid, block, 0, st, p, proj, depth, color, label, origin3_dev, tsdf, weight, color_vol, label_vol);
  else hipLaunchKernelGGL((fusion_integrate_kernel<false, false>), grid, block, 0, st, p, proj, depth, color, label, origin3_dev, tsdf, weight, color_vol, label_vol);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_tsdf_fuse_finish_f32(const float* tsdf, const float* weight, const float* color_vol, int64_t n,
                                          float* tsdf_out, float* color_out, void* stream) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return -22;
  if (n == 0 || (tsdf_out == nullptr && color_out == nullptr)) return 0;
  if (weight == nullptr || (tsdf_out != nullptr && tsdf == nullptr) || (color_out != nullptr && color_vol == nullptr)) return -22;
  hipLaunchKernelGGL(fusion_finish_kernel, dim3((unsigned)ceil_div(n, FUSION_BLOCK)), dim3(FUSION_BLOCK), 0, as_stream(stream),
                     (uint32_t)n, tsdf, weight, color_vol, tsdf_out, color_out);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
