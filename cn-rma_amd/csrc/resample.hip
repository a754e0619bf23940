// TSDF resampling on the device: a volume (and its attribute volumes) read under a rigid transform into a new voxel grid
// (reference: projects/mvsdetection/datasets/tsdf.py:112-180 and data_prepare/scannet/tsdf.py:266-349, TSDF.transform -- an index
// grid, a matrix product, two grid_sample passes and two masked overwrites over the whole volume).  include/cnrma.h (a17) holds the
// contract; the pinned behaviour is that transform ON THE CPU, bit for bit.
//
// One lane owns one OUTPUT voxel (flat index (x ny + y) nz + z: a wave owns a z-run and stores whole lines) and gathers from the
// source.  The transform rows and the two origins are wave-uniform (scalar loads).  A wave whose voxels are all on the border stores
// +1 without touching the source; a wave none of whose nearest samples lies in the truncation band skips the eight corner
// gathers.  No atomics, no reciprocals, no fused operation (the Makefile compiles with -ffp-contract=off), nothing read back to the
// host, no tuning state.
#include <math.h>

#include "common.h"

namespace {

constexpr int RESAMPLE_BLOCK = 256;

struct ResampleParams {
  int X, Y, Z, nx, ny, nz;
  float vs;
};

// the source position of output voxel g in grid_sample's pixel units, s[0..2] along the volume's x, y, z; -> border
__device__ __forceinline__ bool resample_position(const ResampleParams& p, uint32_t g, const float* __restrict__ T,
                                                  const float* __restrict__ src_origin, const float* __restrict__ dst_origin,
                                                  float s[3]) {
  const uint32_t t = g / (uint32_t)p.nz;
  const int k = (int)(g - t * (uint32_t)p.nz), i = (int)(t / (uint32_t)p.ny), j = (int)(t - (uint32_t)i * (uint32_t)p.ny);
  // coords.float() * voxel_size + origin: the product is rounded, then the sum
  const float w0 = (float)i * p.vs + dst_origin[0];
  const float w1 = (float)j * p.vs + dst_origin[1];
  const float w2 = (float)k * p.vs + dst_origin[2];
  const float dims[3] = {(float)p.X, (float)p.Y, (float)p.Z};
  const float last[3] = {(float)(p.X - 1), (float)(p.Y - 1), (float)(p.Z - 1)};
  bool border = false;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    // transform[:3] @ world as the pinned host evaluates it: an un-fused sum from the left
    const float q = ((T[r * 4 + 0] * w0 + T[r * 4 + 1] * w1) + T[r * 4 + 2] * w2) + T[r * 4 + 3] * 1.0f;
    const float c = (q - src_origin[r]) / p.vs;                                   // IEEE division
    const float n = 2.0f * c / last[r] - 1.0f;                                    // [-1, 1] over the old volume, the align_corners way
    border = border || (fabsf(n) >= 1.0f);                                        // a NaN is not on the border
    s[r] = ((n + 1.0f) * dims[r] - 1.0f) / 2.0f;                                  // grid_sample's align_corners=False un-normalisation
  }
  return border;
}

// an index that is safe to load from, whatever f holds (NaN -> 0)
__device__ __forceinline__ uint32_t clamp_index(float f, int dim) { return (uint32_t)fminf(fmaxf(f, 0.0f), (float)(dim - 1)); }

// mode='nearest', padding_mode='zeros': rint with ties to even; the bounds test stays although |n| < 1 (see cnrma.h).
// Indices are 32-bit: the volume has fewer than 2^31 voxels
template <typename T>
__device__ __forceinline__ T sample_nearest(const T* __restrict__ src, const ResampleParams& p, const float s[3]) {
  const float rx = rintf(s[0]), ry = rintf(s[1]), rz = rintf(s[2]);
  const bool in = rx >= 0.0f && rx < (float)p.X && ry >= 0.0f && ry < (float)p.Y && rz >= 0.0f && rz < (float)p.Z;
  const T v = src[(clamp_index(rx, p.X) * (uint32_t)p.Y + clamp_index(ry, p.Y)) * (uint32_t)p.Z + clamp_index(rz, p.Z)];
  return in ? v : (T)0;
}

// mode='bilinear', padding_mode='zeros': ATen's order of corners (volume-z offset fastest), of the weight product and of the sum.
// Bounds, clamped offsets and weights are formed once per axis and side; the eight gathers leave together, from addresses
// that are inside the volume whether the corner is or not, and a corner outside it is left out of the sum
__device__ __forceinline__ float sample_trilinear(const float* __restrict__ src, const ResampleParams& p, const float s[3]) {
  const int dims[3] = {p.X, p.Y, p.Z};
  const uint32_t pitch[3] = {(uint32_t)p.Y * (uint32_t)p.Z, (uint32_t)p.Z, 1u};
  float w[3][2];
  uint32_t off[3][2];
  bool in[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = floorf(s[a]);
    w[a][0] = (f + 1.0f) - s[a];
    w[a][1] = s[a] - f;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const float c = f + (float)d;
      in[a][d] = c >= 0.0f && c < (float)dims[a];
      off[a][d] = clamp_index(c, dims[a]) * pitch[a];
    }
  }
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = src[off[0][c >> 2] + off[1][(c >> 1) & 1] + off[2][c & 1]];
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float weight = (w[2][c & 1] * w[1][(c >> 1) & 1]) * w[0][c >> 2];
    const float sum = acc + v[c] * weight;
    acc = (in[0][c >> 2] && in[1][(c >> 1) & 1] && in[2][c & 1]) ? sum : acc;
  }
  return acc;
}

__global__ __launch_bounds__(RESAMPLE_BLOCK) void tsdf_resample_kernel(ResampleParams p, const float* __restrict__ src,
                                                                       const float* __restrict__ T,
                                                                       const float* __restrict__ src_origin,
                                                                       const float* __restrict__ dst_origin,
                                                                       float* __restrict__ dst) {
  const uint32_t N = (uint32_t)p.nx * (uint32_t)p.ny * (uint32_t)p.nz;             // < 2^31 (checked by the entry point)
  const uint32_t g = blockIdx.x * (uint32_t)RESAMPLE_BLOCK + threadIdx.x;
  if (g >= N) return;
  float s[3];
  const bool border = resample_position(p, g, T, src_origin, dst_origin, s);
  if (__ballot(!border) == 0ull) {                                                 // the whole wave lies outside the old volume
    dst[g] = 1.0f;
    return;
  }
  float out = 1.0f;
  bool band = false;
  if (!border) {
    out = sample_nearest<float>(src, p, s);
    band = fabsf(out) < 1.0f;
  }
  if (__ballot(band) != 0ull) {                                                    // else: no lane of the wave needs the corners
    if (band) out = sample_trilinear(src, p, s);
  }
  dst[g] = out;
}

__global__ __launch_bounds__(RESAMPLE_BLOCK) void tsdf_resample_attr_f32_kernel(ResampleParams p, int C,
                                                                                const float* __restrict__ src,
                                                                                const float* __restrict__ T,
                                                                                const float* __restrict__ src_origin,
                                                                                const float* __restrict__ dst_origin,
                                                                                float* __restrict__ dst) {
  const uint32_t N = (uint32_t)p.nx * (uint32_t)p.ny * (uint32_t)p.nz;
  const uint32_t g = blockIdx.x * (uint32_t)RESAMPLE_BLOCK + threadIdx.x;
  if (g >= N) return;
  float s[3];
  resample_position(p, g, T, src_origin, dst_origin, s);
  const size_t S = (size_t)p.X * p.Y * p.Z;
  for (int c = 0; c < C; ++c) dst[(size_t)c * N + g] = sample_trilinear(src + (size_t)c * S, p, s);
}

__global__ __launch_bounds__(RESAMPLE_BLOCK) void tsdf_resample_attr_i64_kernel(ResampleParams p, int C,
                                                                                const int64_t* __restrict__ src,
                                                                                const float* __restrict__ T,
                                                                                const float* __restrict__ src_origin,
                                                                                const float* __restrict__ dst_origin,
                                                                                int64_t border_fill, int fill,
                                                                                int64_t* __restrict__ dst) {
  const uint32_t N = (uint32_t)p.nx * (uint32_t)p.ny * (uint32_t)p.nz;
  const uint32_t g = blockIdx.x * (uint32_t)RESAMPLE_BLOCK + threadIdx.x;
  if (g >= N) return;
  float s[3];
  const bool border = resample_position(p, g, T, src_origin, dst_origin, s);
  const size_t S = (size_t)p.X * p.Y * p.Z;
  for (int c = 0; c < C; ++c)
    dst[(size_t)c * N + g] = (fill != 0 && border) ? border_fill : sample_nearest<int64_t>(src + (size_t)c * S, p, s);
}

// 0: launch, 1: nothing to do, -22: refused
int resample_check(const void* src, int C, int X, int Y, int Z, const void* src_origin, const void* transform, const void* dst_origin,
                   int nx, int ny, int nz, const void* dst) {
  if (C < 0 || nx < 0 || ny < 0 || nz < 0) return -22;
  if (X < 2 || Y < 2 || Z < 2) return -22;                                          // the normalisation divides by dim - 1
  const int64_t S = (int64_t)X * Y * Z, N = (int64_t)nx * ny * nz, lim = (int64_t)1 << 31;
  if (S >= lim || N >= lim) return -22;
  if (src == nullptr || src_origin == nullptr || transform == nullptr || dst_origin == nullptr) return -22;
  if (N == 0 || C == 0) return 1;
  if (dst == nullptr) return -22;
  return 0;
}

}  // namespace

extern "C" int cnrma_tsdf_resample_f32(const float* src, int X, int Y, int Z, const float* src_origin3_dev, float voxel_size,
                                       const float* transform12_dev, const float* dst_origin3_dev, int nx, int ny, int nz,
                                       float* dst, void* stream) {
  const int rc = resample_check(src, 1, X, Y, Z, src_origin3_dev, transform12_dev, dst_origin3_dev, nx, ny, nz, dst);
  if (rc != 0) return rc < 0 ? rc : 0;
  const ResampleParams p{X, Y, Z, nx, ny, nz, voxel_size};
  const int64_t N = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_resample_kernel, dim3((unsigned)ceil_div(N, RESAMPLE_BLOCK)), dim3(RESAMPLE_BLOCK), 0, as_stream(stream),
                     p, src, transform12_dev, src_origin3_dev, dst_origin3_dev, dst);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_tsdf_resample_attr_f32(const float* src, int C, int X, int Y, int Z, const float* src_origin3_dev,
                                            float voxel_size, const float* transform12_dev, const float* dst_origin3_dev, int nx,
                                            int ny, int nz, float* dst, void* stream) {
  const int rc = resample_check(src, C, X, Y, Z, src_origin3_dev, transform12_dev, dst_origin3_dev, nx, ny, nz, dst);
  if (rc != 0) return rc < 0 ? rc : 0;
  const ResampleParams p{X, Y, Z, nx, ny, nz, voxel_size};
  const int64_t N = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_resample_attr_f32_kernel, dim3((unsigned)ceil_div(N, RESAMPLE_BLOCK)), dim3(RESAMPLE_BLOCK), 0,
                     as_stream(stream), p, C, src, transform12_dev, src_origin3_dev, dst_origin3_dev, dst);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_tsdf_resample_attr_i64(const int64_t* src, int C, int X, int Y, int Z, const float* src_origin3_dev,
                                            float voxel_size, const float* transform12_dev, const float* dst_origin3_dev, int nx,
                                            int ny, int nz, int64_t border_fill, int fill_border, int64_t* dst, void* stream) {
  const int rc = resample_check(src, C, X, Y, Z, src_origin3_dev, transform12_dev, dst_origin3_dev, nx, ny, nz, dst);
  if (rc != 0) return rc < 0 ? rc : 0;
  const ResampleParams p{X, Y, Z, nx, ny, nz, voxel_size};
  const int64_t N = (int64_t)nx * ny * nz;
  hipLaunchKernelGGL(tsdf_resample_attr_i64_kernel, dim3((unsigned)ceil_div(N, RESAMPLE_BLOCK)), dim3(RESAMPLE_BLOCK), 0,
                     as_stream(stream), p, C, src, transform12_dev, src_origin3_dev, dst_origin3_dev, border_fill, fill_border, dst);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
