// libcnrma_unet_hip.so (include/cnrma_unet.h): the dense 3x3x3 convolutions of the Atlas 3D U-Net as an implicit GEMM in f16x3.
//
// unet_conv3_kernel<STRIDE, VT, NT, WAVES>: a workgroup owns a box of output voxels -- 4 (y) x 8 (z) = 32 voxels form one matrix-pipe
// column tile, WAVES * VT such tiles lie along x -- and NT * 32 output channels.  Per chunk of 16 input channels it loads the box's
// halo once (reads run along z), splits every element to its fp16 halves h, m once, and writes a voxel-major, channel-minor LDS
// image: the 8 channels a lane's B fragment holds are 16 contiguous bytes (one ds_read_b128), and the 27 taps of the chunk are 27
// compile-time offsets into the same image.  Halo positions outside the volume are written as zeros, never loaded.  The weights
// are the A operand (rows = output channels), read straight from the prepared fragment image, so the accumulator has the voxel on
// the lane and a store instruction writes runs along z.  K order: chunks ascending, taps ascending inside a chunk, m*h, h*m, h*h
// per step -- fixed, and no atomics touch y, so a result is reproducible bit for bit.
#include <math.h>

#include "../../include/cnrma_unet.h"
#include "f16x3.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int KC = 16;                       // input channels per chunk: one k step of the 32x32x16 product
constexpr int TY = 4, TZ = 8;                // a column tile: 32 output voxels at one x
constexpr int HEAD_U4 = 4;                   // the image's 64-byte head {sw, 1 / sw}, in 16-byte units
static_assert(CNRMA_UNET_BOUND_WORDS == AMAX_SLOTS * AMAX_STRIDE, "the bound convention of f16x3.h");

template <int STRIDE, int VT, int WAVES>
struct Box {
  static constexpr int TX = WAVES * VT;
  static constexpr int HX = (TX - 1) * STRIDE + 3, HY = (TY - 1) * STRIDE + 3, HZ = (TZ - 1) * STRIDE + 3;
  static constexpr int NHV = HX * HY * HZ;   // halo voxels; LDS = NHV * 64 bytes
};

__global__ __launch_bounds__(256) void unet_absmax_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ bound) {
  float mx = 0.0f;
  const bool vec = (((uintptr_t)x) & 15) == 0;
  for (int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; t < n; t += (int64_t)gridDim.x * blockDim.x * 4) {
    if (vec && t + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(x + t);
      mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fmaxf(fabsf(v.y), fabsf(v.z)), fabsf(v.w)));
    } else {
      for (int j = 0; j < 4 && t + j < n; ++j) mx = fmaxf(mx, fabsf(x[t + j]));
    }
  }
  __shared__ float sh[4];
  block_amax_publish<4>(bound, mx, sh);
}

// one workgroup: max|w| -> the image's head {sw, 1 / sw, 0...}
__global__ __launch_bounds__(1024) void unet_weight_scale_kernel(const float* __restrict__ w, int64_t n, float* __restrict__ head) {
  float mx = 0.0f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) mx = fmaxf(mx, fabsf(w[i]));
  mx = wave_max(mx);
  __shared__ float sh[16];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x < 16) {
    float m = sh[0];
    for (int i = 1; i < 16; ++i) m = fmaxf(m, sh[i]);
    const float s = f16_scale_for(m);
    head[threadIdx.x] = threadIdx.x == 0 ? s : (threadIdx.x == 1 ? 1.0f / s : 0.0f);
  }
}

// one thread per (cout tile, chunk, tap, lane): its 8 weights -> the h and the m fragment.  Lane l of a fragment holds row
// cout = 32 ct + (l & 31), k = cin = 16 kc + 8 (l >> 5) + j in element j (the A operand of the 32x32x16 product)
__global__ __launch_bounds__(256) void unet_weight_pack_kernel(const float* __restrict__ w, int Cin, int Cout, uint4* image) {
  const int nkc = Cin / KC;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)(Cout / 32) * nkc * 27 * 64) return;
  const int lane = (int)(t & 63);
  int f = (int)(t >> 6);
  const int tap = f % 27;
  f /= 27;
  const int kc = f % nkc, ct = f / nkc;
  const int cout = ct * 32 + (lane & 31), cin0 = kc * KC + 8 * (lane >> 5);
  const float sw = reinterpret_cast<const float*>(image)[0];
  uint16_t h[8], m[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) split2_f16(w[((int64_t)cout * Cin + cin0 + j) * 27 + tap] * sw, h[j], m[j]);
  uint4* frag = image + HEAD_U4 + ((int64_t)(ct * nkc + kc) * 27 + tap) * 2 * 64;
  frag[lane] = make_uint4(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16), h[4] | ((uint32_t)h[5] << 16),
                          h[6] | ((uint32_t)h[7] << 16));
  frag[64 + lane] = make_uint4(m[0] | ((uint32_t)m[1] << 16), m[2] | ((uint32_t)m[3] << 16), m[4] | ((uint32_t)m[5] << 16),
                               m[6] | ((uint32_t)m[7] << 16));
}

// grid: x = spatial boxes (x-major, z fastest), y = slices of NT * 32 output channels, z = batch item
template <int STRIDE, int VT, int NT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void unet_conv3_kernel(const float* __restrict__ x, const float* __restrict__ bound_x,
                                                                const uint4* __restrict__ image, const float* __restrict__ scale,
                                                                const float* __restrict__ shift, const float* residual, int relu,
                                                                int Cin, int Cout, int X, int Y, int Z, int OX, int OY, int OZ,
                                                                int nby, int nbz, float* y, float* bound_y) {
  using G = Box<STRIDE, VT, WAVES>;
  constexpr int HY = G::HY, HZ = G::HZ, NHV = G::NHV;
  __shared__ uint4 img[2][NHV][2];           // [h, m][halo voxel][channels 0-7, 8-15 of the chunk]
  __shared__ float sh_max[WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
  const int oyl = r >> 3, ozl = r & 7;
  int t = blockIdx.x;
  const int bz = t % nbz;
  t /= nbz;
  const int by = t % nby, bx = t / nby;
  const int ox0 = bx * G::TX, oy0 = by * TY, oz0 = bz * TZ;
  const int ix0 = ox0 * STRIDE - 1, iy0 = oy0 * STRIDE - 1, iz0 = oz0 * STRIDE - 1;
  const int b = blockIdx.z, ct0 = blockIdx.y * NT, nkc = Cin / KC;
  const int64_t cstride = (int64_t)X * Y * Z;
  const float* xb = x + (int64_t)b * Cin * cstride;
  const float sx = f16_scale_for(read_amax(bound_x));
  const uint4* frags = image + HEAD_U4;
  const int lane_hv = ((wave * VT * STRIDE) * HY + oyl * STRIDE) * HZ + ozl * STRIDE;

  f32x16_t acc[VT][NT];
#pragma unroll
  for (int v = 0; v < VT; ++v)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[v][n][i] = 0.0f;

  for (int kc = 0; kc < nkc; ++kc) {
    __syncthreads();                         // the previous chunk's fragment reads are done
    for (int i = tid; i < 2 * NHV; i += 64 * WAVES) {
      const int g = i / NHV, hv = i - g * NHV;
      const int hz = hv % HZ, hy = (hv / HZ) % HY, hx = hv / (HZ * HY);
      const int ix = ix0 + hx, iy = iy0 + hy, iz = iz0 + hz;
      float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
      if ((unsigned)ix < (unsigned)X && (unsigned)iy < (unsigned)Y && (unsigned)iz < (unsigned)Z) {
        const float* p = xb + (int64_t)(kc * KC + g * 8) * cstride + ((int64_t)ix * Y + iy) * Z + iz;
        lo = make_float4(p[0], p[cstride], p[2 * cstride], p[3 * cstride]);
        hi = make_float4(p[4 * cstride], p[5 * cstride], p[6 * cstride], p[7 * cstride]);
      }
      uint2 h0, m0, h1, m1;
      split2(lo, sx, h0, m0);
      split2(hi, sx, h1, m1);
      img[0][hv][g] = make_uint4(h0.x, h0.y, h1.x, h1.y);
      img[1][hv][g] = make_uint4(m0.x, m0.y, m1.x, m1.y);
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 27; ++tap) {
      const int dx = tap / 9, dy = (tap / 3) % 3, dz = tap % 3;
      f16x8_t xh[VT], xm[VT];
#pragma unroll
      for (int v = 0; v < VT; ++v) {
        const int hv = lane_hv + ((v * STRIDE + dx) * HY + dy) * HZ + dz;
        xh[v] = __builtin_bit_cast(f16x8_t, img[0][hv][half]);
        xm[v] = __builtin_bit_cast(f16x8_t, img[1][hv][half]);
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const uint4* f = frags + ((int64_t)((ct0 + n) * nkc + kc) * 27 + tap) * 2 * 64 + lane;
        const f16x8_t wh = __builtin_bit_cast(f16x8_t, f[0]), wm = __builtin_bit_cast(f16x8_t, f[64]);
#pragma unroll
        for (int v = 0; v < VT; ++v) {
          f32x16_t c = acc[v][n];
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wm, xh[v], c, 0, 0, 0);    // m*h
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xm[v], c, 0, 0, 0);    // h*m
          c = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh[v], c, 0, 0, 0);    // h*h
          acc[v][n] = c;
        }
      }
    }
  }

  // epilogue: accumulator register i of a tile is output channel (i & 3) + 8 (i >> 2) + 4 (lane >> 5), the lane's voxel its column
  const float inv_sx = 1.0f / sx, inv_sw = reinterpret_cast<const float*>(image)[1];
  const int oy = oy0 + oyl, oz = oz0 + ozl;
  float mx = 0.0f;
#pragma unroll
  for (int v = 0; v < VT; ++v) {
    const int ox = ox0 + wave * VT + v;
    if (ox < OX && oy < OY && oz < OZ) {
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int c = (ct0 + n) * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
          const int64_t idx = ((((int64_t)b * Cout + c) * OX + ox) * OY + oy) * OZ + oz;
          float val = acc[v][n][i] * inv_sx * inv_sw;
          if (scale != nullptr) val = val * scale[c] + shift[c];
          if (residual != nullptr) val += residual[idx];
          if (relu) val = fmaxf(val, 0.0f);
          y[idx] = val;
          mx = fmaxf(mx, fabsf(val));
        }
    }
  }
  if (bound_y != nullptr) block_amax_publish<WAVES>(bound_y, mx, sh_max);
}

bool widths_ok(int Cin, int Cout) {
  return Cin >= 32 && Cin <= 256 && Cin % 32 == 0 && Cout >= 32 && Cout <= 256 && Cout % 32 == 0;
}

bool shape_ok(int B, int Cin, int Cout, int X, int Y, int Z, int stride) {
  if (!widths_ok(Cin, Cout) || (stride != 1 && stride != 2) || B < 1 || B > 65535 || X < 1 || Y < 1 || Z < 1) return false;
  const int64_t lim = (int64_t)1 << 31;
  if (X >= lim / Y || (int64_t)X * Y >= lim / Z || (int64_t)X * Y * Z >= lim / ((int64_t)B * (Cin > Cout ? Cin : Cout))) return false;
  return true;
}

template <int STRIDE, int VT, int NT, int WAVES>
int launch_conv3(const float* x, const float* bound_x, const void* image, const float* scale, const float* shift,
                 const float* residual, int relu, int B, int Cin, int Cout, int X, int Y, int Z, float* y, float* bound_y,
                 hipStream_t st) {
  using G = Box<STRIDE, VT, WAVES>;
  const int OX = (X - 1) / STRIDE + 1, OY = (Y - 1) / STRIDE + 1, OZ = (Z - 1) / STRIDE + 1;
  const int nbx = (OX + G::TX - 1) / G::TX, nby = (OY + TY - 1) / TY, nbz = (OZ + TZ - 1) / TZ;
  const dim3 grid((unsigned)(nbx * nby * nbz), (unsigned)(Cout / (32 * NT)), (unsigned)B);
  hipLaunchKernelGGL((unet_conv3_kernel<STRIDE, VT, NT, WAVES>), grid, dim3(64 * WAVES), 0, st, x, bound_x,
                     reinterpret_cast<const uint4*>(image), scale, shift, residual, relu, Cin, Cout, X, Y, Z, OX, OY, OZ, nby, nbz, y,
                     bound_y);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int cnrma_unet_abi_version(void) { return CNRMA_UNET_ABI_VERSION; }

int cnrma_unet_conv3_supported(int B, int Cin, int Cout, int X, int Y, int Z, int stride) {
  return shape_ok(B, Cin, Cout, X, Y, Z, stride) ? 1 : 0;
}

size_t cnrma_unet_conv3_weight_bytes(int Cin, int Cout) {
  return widths_ok(Cin, Cout) ? (size_t)HEAD_U4 * 16 + (size_t)Cout * Cin * 27 * 4 : 0;
}

int cnrma_unet_conv3_prepare_weights(const float* w, int Cin, int Cout, void* image, void* stream) {
  if (!widths_ok(Cin, Cout) || w == nullptr || image == nullptr || ((uintptr_t)image & 15) != 0) return CNRMA_UNET_EINVAL;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(unet_weight_scale_kernel, dim3(1), dim3(1024), 0, st, w, (int64_t)Cout * Cin * 27, reinterpret_cast<float*>(image));
  CNRMA_LAUNCH_CHECK();
  const int64_t threads = (int64_t)(Cout / 32) * (Cin / KC) * 27 * 64;
  hipLaunchKernelGGL(unet_weight_pack_kernel, dim3((unsigned)ceil_div(threads, 256)), dim3(256), 0, st, w, Cin, Cout,
                     reinterpret_cast<uint4*>(image));
  CNRMA_LAUNCH_CHECK();
  return 0;
}

int cnrma_unet_absmax_f32(const float* x, int64_t n, float* bound, void* stream) {
  if (n < 0 || (n > 0 && x == nullptr) || bound == nullptr) return CNRMA_UNET_EINVAL;
  hipStream_t st = as_stream(stream);
  hipError_t e = cnrma_fill_bytes(bound, 0, (size_t)CNRMA_UNET_BOUND_WORDS * 4, st);
  if (e != hipSuccess) return -(int)e;
  if (n == 0) return 0;
  int64_t blocks = ceil_div(n, 256 * 4 * 8);
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(unet_absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, bound);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

int cnrma_unet_conv3_forward(const float* x, const float* bound_x, const void* image, const float* scale, const float* shift,
                             const float* residual, int relu, int stride, int B, int Cin, int Cout, int X, int Y, int Z, float* y,
                             float* bound_y, void* stream) {
  if (!shape_ok(B, Cin, Cout, X, Y, Z, stride) || x == nullptr || bound_x == nullptr || image == nullptr || y == nullptr ||
      ((uintptr_t)image & 15) != 0 || (scale != nullptr && shift == nullptr))
    return CNRMA_UNET_EINVAL;
  hipStream_t st = as_stream(stream);
  if (bound_y != nullptr) {
    hipError_t e = cnrma_fill_bytes(bound_y, 0, (size_t)CNRMA_UNET_BOUND_WORDS * 4, st);
    if (e != hipSuccess) return -(int)e;
  }
  const bool wide = Cout % 64 == 0;          // two channel tiles per wave share every voxel fragment
  if (stride == 1)
    return wide ? launch_conv3<1, 2, 2, 4>(x, bound_x, image, scale, shift, residual, relu, B, Cin, Cout, X, Y, Z, y, bound_y, st)
                : launch_conv3<1, 2, 1, 4>(x, bound_x, image, scale, shift, residual, relu, B, Cin, Cout, X, Y, Z, y, bound_y, st);
  return wide ? launch_conv3<2, 1, 2, 2>(x, bound_x, image, scale, shift, residual, relu, B, Cin, Cout, X, Y, Z, y, bound_y, st)
              : launch_conv3<2, 1, 1, 2>(x, bound_x, image, scale, shift, residual, relu, B, Cin, Cout, X, Y, Z, y, bound_y, st);
}

}  // extern "C"
