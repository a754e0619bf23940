// libcnrma_unetjoin_hip.so (include/cnrma_unet_join.h): the decoder joints of the Atlas 3D U-Net, one fused pass per level.
//
// out = (u + max(scale * (observed ? p : u) + shift, 0)) / 2 with u = w_up . trilinear_x2(xc) and p = w_proj . e, in exact fp32 on
// the matrix pipe (32x32x2 fp32 products).  Two kernels per joint:
//   unetjoin_up_kernel    v = w_up . xc on the COARSE grid (the interpolation's weights sum to one, so it commutes with a 1x1x1
//                         convolution: an eighth of the products).  Weights are the A operand, 32 flat voxels lie on the lanes.
//   unetjoin_fuse_kernel  a workgroup owns 4 (x) x 4 (y) x 32 (z) fine voxels and 32 output channels: it stages its 32 rows of w_proj in
//                         LDS, computes p over e with the voxel on the lane (reads and stores run along z), then stages its coarse
//                         tile of v with the one-voxel halo (4 x 4 x 18, positions outside the volume clamped by coordinate) over
//                         the weights, forms u from the eight taps and applies select / affine / ReLU / mean in registers.
//                         One atomic maximum per workgroup publishes max|out| (the bound convention of f16x3.h); nothing else is
//                         atomic, so a result is reproducible bit for bit.
// unetjoin_observed_kernel reads the network's input once for the observed mask and its magnitude bound.
#include <math.h>

#include "../../include/cnrma_unet.h"
#include "../../include/cnrma_unet_join.h"
#include "f16x3.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

constexpr int WAVES = 4;
constexpr int UP_VT = 2, VT = 4;             // a wave owns UP_VT (up kernel) / VT (fuse kernel) column tiles of 32 voxels
constexpr int UP_KB = 8, KB = 4;             // k steps (of 2 channels) whose operand loads leave together: 16 loads per wave in flight
constexpr int WPAD = 33;                     // LDS weight image [k][32 rows], padded: the transposing writes spread over the banks
constexpr int TX = VT, TY = WAVES, TZ = 32;  // fuse kernel: wave = y row, column tile = x, lane = z
constexpr int HX = TX / 2 + 2, HY = TY / 2 + 2, HZ = TZ / 2 + 2, CHS = HX * HY * HZ;     // coarse halo tile of one channel
constexpr int STAGE_IT = 32 * CHS / (64 * WAVES), STAGE_BATCH = 9;          // halo loads per thread, and how many leave together
static_assert(32 * CHS % (64 * WAVES) == 0 && STAGE_IT % STAGE_BATCH == 0, "the halo tile is dealt to the threads in whole batches");
static_assert(CNRMA_UNET_JOIN_BOUND_WORDS == AMAX_SLOTS * AMAX_STRIDE, "the bound convention of f16x3.h");
static_assert(CNRMA_UNET_JOIN_BOUND_WORDS == CNRMA_UNET_BOUND_WORDS, "one bound convention for the U-Net's two libraries");

// rows c0 .. c0 + 31 of w [rows][K] -> sw[k * WPAD + row]: lane l of an A operand reads sw[(k + (l >> 5)) * WPAD + (l & 31)]
__device__ __forceinline__ void unetjoin_stage_weights(const float* __restrict__ w, int K, int c0, float* sw) {
  for (int i = threadIdx.x; i < 32 * K; i += 64 * WAVES) {
    const int r = i / K, k = i - r * K;
    sw[k * WPAD + r] = w[(int64_t)(c0 + r) * K + k];
  }
}

// one axis of the x2 trilinear up-sampling (align_corners = false): output index o of a coarse axis of length n reads i0 and i1 with
// weights 1 - lam and lam; src = max(o / 2 - 0.25, 0), i0 = floor(src), i1 = min(i0 + 1, n - 1), lam = src - i0
__device__ __forceinline__ void unetjoin_taps(int o, int n, int& i0, int& i1, float& lam) {
  i0 = o > 0 ? (o - 1) >> 1 : 0;
  lam = o > 0 ? ((o & 1) ? 0.25f : 0.75f) : 0.0f;
  i1 = i0 + 1 < n ? i0 + 1 : n - 1;
}

// grid: x = tiles of WAVES * UP_VT * 32 flat coarse voxels, y = tiles of 32 output channels, z = batch item; LDS: Cc * WPAD floats
__global__ __launch_bounds__(64 * WAVES) void unetjoin_up_kernel(const float* __restrict__ xc, const float* __restrict__ w_up, int Cc,
                                                                 int Cf, int Nc, float* __restrict__ v) {
  extern __shared__ float sw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
  const int c0 = blockIdx.y * 32, b = blockIdx.z;
  unetjoin_stage_weights(w_up, Cc, c0, sw);
  __syncthreads();
  const float* xb = xc + (int64_t)b * Cc * Nc + (int64_t)half * Nc;
  int n[UP_VT], nl[UP_VT];
  f32x16_t acc[UP_VT];
#pragma unroll
  for (int t = 0; t < UP_VT; ++t) {
    n[t] = ((int)blockIdx.x * WAVES + wave) * (UP_VT * 32) + t * 32 + r;
    nl[t] = n[t] < Nc ? n[t] : Nc - 1;       // a tail lane reads the last voxel again; its column is never stored
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
  }
  const float* swl = sw + half * WPAD + r;
  for (int k0 = 0; k0 < Cc; k0 += 2 * UP_KB) {              // Cc is a multiple of 32: whole batches; a batch's loads leave together
    float a[UP_KB], x[UP_KB][UP_VT];
#pragma unroll
    for (int j = 0; j < UP_KB; ++j) {
      a[j] = swl[(k0 + 2 * j) * WPAD];
#pragma unroll
      for (int t = 0; t < UP_VT; ++t) x[j][t] = xb[(int64_t)(k0 + 2 * j) * Nc + nl[t]];
    }
#pragma unroll
    for (int j = 0; j < UP_KB; ++j)
#pragma unroll
      for (int t = 0; t < UP_VT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[j][t], acc[t], 0, 0, 0);
  }
  // accumulator register i is output channel (i & 3) + 8 (i >> 2) + 4 (lane >> 5), the lane's voxel its column
#pragma unroll
  for (int t = 0; t < UP_VT; ++t)
    if (n[t] < Nc) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = c0 + (i & 3) + 8 * (i >> 2) + 4 * half;
        v[((int64_t)b * Cf + c) * Nc + n[t]] = acc[t][i];
      }
    }
}

// grid: x = (spatial tiles, x-major, z fastest) * (Cf / 32) with the channel tile fastest (the workgroups that read the same voxels of
// e are dispatched together), z = batch item; LDS: max(32 * CHS, Cf * WPAD) floats, the weights first and the halo tile over them
__global__ __launch_bounds__(64 * WAVES, 4) void unetjoin_fuse_kernel(const float* __restrict__ v, const float* __restrict__ e,
                                                                   const float* __restrict__ w_proj, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift,
                                                                   const unsigned char* __restrict__ observed, int step, int Cf,
                                                                   int Xc, int Yc, int Zc, int nct, int nby, int nbz,
                                                                   float* __restrict__ out, float* bound_out) {
  extern __shared__ float smem[];
  float* sw = smem;                          // [Cf][WPAD], during the product
  float* sv = smem;                          // [32 channels][HX][HY][HZ], after it
  __shared__ float sh_max[WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, half = lane >> 5;
  int t = blockIdx.x;
  const int c0 = (t % nct) * 32;
  t /= nct;
  const int bz = t % nbz;
  t /= nbz;
  const int by = t % nby, bx = t / nby;
  const int fx0 = bx * TX, fy0 = by * TY, fz0 = bz * TZ;
  const int X = 2 * Xc, Y = 2 * Yc, Z = 2 * Zc, b = blockIdx.z;
  const int cx0 = fx0 / 2 - 1, cy0 = fy0 / 2 - 1, cz0 = fz0 / 2 - 1;

  unetjoin_stage_weights(w_proj, Cf, c0, sw);
  __syncthreads();

  // the wave's VT column tiles: fine voxels (fx0 + q, fy0 + wave, fz0 + r).  A voxel past the volume reads the last one of its axis
  // again (its column of the product is its own and is never stored)
  const int plane = X * Y * Z;
  const int fy = fy0 + wave, fz = fz0 + r;
  const int fyl = min(fy, Y - 1), fzl = min(fz, Z - 1);
  const float* eb = e + (int64_t)b * Cf * plane + (int64_t)half * plane;
  int off[VT];
  f32x16_t acc[VT];
#pragma unroll
  for (int q = 0; q < VT; ++q) {
    off[q] = (min(fx0 + q, X - 1) * Y + fyl) * Z + fzl;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.0f;
  }
  const float* swl = sw + half * WPAD + r;
  for (int k0 = 0; k0 < Cf; k0 += 2 * KB) {                 // Cf is a multiple of 32: whole batches; a batch's loads leave together
    float a[KB], x[KB][VT];
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      a[j] = swl[(k0 + 2 * j) * WPAD];
#pragma unroll
      for (int q = 0; q < VT; ++q) x[j][q] = eb[(int64_t)(k0 + 2 * j) * plane + off[q]];
    }
#pragma unroll
    for (int j = 0; j < KB; ++j)
#pragma unroll
      for (int q = 0; q < VT; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], x[j][q], acc[q], 0, 0, 0);
  }

  // the coarse tile of v over the weights: STAGE_BATCH loads leave together, then their LDS writes
  __syncthreads();
  const float* vb = v + ((int64_t)b * Cf + c0) * ((int64_t)Xc * Yc * Zc);
  for (int it = 0; it < STAGE_IT; it += STAGE_BATCH) {
    float held[STAGE_BATCH];
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) {
      const int i = tid + (it + j) * (64 * WAVES);
      const int c = i / CHS, h = i - c * CHS;
      const int hz = h % HZ, hy = (h / HZ) % HY, hx = h / (HZ * HY);
      const int cx = min(max(cx0 + hx, 0), Xc - 1), cy = min(max(cy0 + hy, 0), Yc - 1), cz = min(max(cz0 + hz, 0), Zc - 1);
      held[j] = vb[(((int64_t)c * Xc + cx) * Yc + cy) * Zc + cz];
    }
#pragma unroll
    for (int j = 0; j < STAGE_BATCH; ++j) sv[tid + (it + j) * (64 * WAVES)] = held[j];
  }
  __syncthreads();

  // epilogue: accumulator register i of a tile is output channel (i & 3) + 8 (i >> 2) + 4 (lane >> 5), the lane's voxel its column
  int y0, y1, z0, z1;
  float ly, lz;
  unetjoin_taps(fyl, Yc, y0, y1, ly);
  unetjoin_taps(fzl, Zc, z0, z1, lz);
  y0 -= cy0, y1 -= cy0, z0 -= cz0, z1 -= cz0;
  const float wy0 = 1.0f - ly, wz0 = 1.0f - lz;
  const float* svl = sv + 4 * half * CHS;
  const int X0 = step * X, Y0 = step * Y, Z0 = step * Z;
  float mx = 0.0f;
#pragma unroll
  for (int q = 0; q < VT; ++q) {
    const int fx = fx0 + q;
    if (fx < X && fy < Y && fz < Z) {
      int x0, x1;
      float lx;
      unetjoin_taps(fx, Xc, x0, x1, lx);
      x0 -= cx0, x1 -= cx0;
      const float wx0 = 1.0f - lx;
      const int o00 = (x0 * HY + y0) * HZ, o01 = (x0 * HY + y1) * HZ, o10 = (x1 * HY + y0) * HZ, o11 = (x1 * HY + y1) * HZ;
      bool seen = true;
      if (observed != nullptr)
        seen = observed[(((int64_t)b * X0 + (int64_t)step * fx) * Y0 + (int64_t)step * fy) * Z0 + (int64_t)step * fz] != 0;
      const int64_t o = ((int64_t)b * Cf + c0 + 4 * half) * plane + ((int64_t)fx * Y + fy) * Z + fz;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int cl = (i & 3) + 8 * (i >> 2);               // + 4 * half: in svl, o and the channel below
        const float* s = svl + cl * CHS;
        const float t00 = wz0 * s[o00 + z0] + lz * s[o00 + z1], t01 = wz0 * s[o01 + z0] + lz * s[o01 + z1];
        const float t10 = wz0 * s[o10 + z0] + lz * s[o10 + z1], t11 = wz0 * s[o11 + z0] + lz * s[o11 + z1];
        const float u = wx0 * (wy0 * t00 + ly * t01) + lx * (wy0 * t10 + ly * t11);
        float sel = seen ? acc[q][i] : u;
        if (scale != nullptr) {
          const int c = c0 + cl + 4 * half;
          sel = sel * scale[c] + shift[c];
        }
        const float val = (u + fmaxf(sel, 0.0f)) * 0.5f;
        out[o + (int64_t)cl * plane] = val;
        mx = fmaxf(mx, fabsf(val));
      }
    }
  }
  if (bound_out != nullptr) block_amax_publish<WAVES>(bound_out, mx, sh_max);
}

// grid: x = tiles of 256 * 4 voxels, y = batch item.  A thread owns four consecutive voxels of one item over every channel
__global__ __launch_bounds__(256) void unetjoin_observed_kernel(const float* __restrict__ x, int C, int N,
                                                                unsigned char* __restrict__ observed, float* bound_x) {
  const int b = blockIdx.y;
  const int n0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
  const float* xb = x + (int64_t)b * C * N;
  unsigned char* ob = observed + (int64_t)b * N;
  float mx = 0.0f;
  if (n0 < N) {
    unsigned any = 0;
    if ((N & 3) == 0 && (((uintptr_t)x) & 15) == 0) {        // every channel plane starts on 16 bytes, and n0 + 3 < N
#pragma unroll 8
      for (int c = 0; c < C; ++c) {
        const float4 t = *reinterpret_cast<const float4*>(xb + (int64_t)c * N + n0);
        any |= (t.x != 0.0f ? 1u : 0u) | (t.y != 0.0f ? 0x100u : 0u) | (t.z != 0.0f ? 0x10000u : 0u) | (t.w != 0.0f ? 0x1000000u : 0u);
        mx = fmaxf(fmaxf(mx, fabsf(t.x)), fmaxf(fmaxf(fabsf(t.y), fabsf(t.z)), fabsf(t.w)));
      }
    } else {
      for (int c = 0; c < C; ++c)
        for (int j = 0; j < 4 && n0 + j < N; ++j) {
          const float t = xb[(int64_t)c * N + n0 + j];
          any |= t != 0.0f ? 1u << (8 * j) : 0u;
          mx = fmaxf(mx, fabsf(t));
        }
    }
    if ((N & 3) == 0 && (((uintptr_t)observed) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(ob + n0) = any;
    } else {
      for (int j = 0; j < 4 && n0 + j < N; ++j) ob[n0 + j] = (unsigned char)((any >> (8 * j)) & 1u);
    }
  }
  __shared__ float sh[4];
  if (bound_x != nullptr) block_amax_publish<4>(bound_x, mx, sh);
}

bool widths_ok(int Cc, int Cf) {
  return Cc >= 32 && Cc <= 256 && Cc % 32 == 0 && Cf >= 32 && Cf <= 256 && Cf % 32 == 0;
}

// out = B * Cf * 8 * Xc * Yc * Zc elements, below 2^31 (e is as large; xc and the scratch are smaller: Cc <= 256 = 8 * 32 <= 8 * Cf)
bool shape_ok(int B, int Cc, int Cf, int Xc, int Yc, int Zc) {
  if (!widths_ok(Cc, Cf) || B < 1 || B > 65535 || Xc < 1 || Yc < 1 || Zc < 1) return false;
  const int64_t lim = ((int64_t)1 << 31) / 8;
  if (Xc >= lim / Yc || (int64_t)Xc * Yc >= lim / Zc || (int64_t)Xc * Yc * Zc >= lim / ((int64_t)B * Cf)) return false;
  return true;
}

}  // namespace

extern "C" {

int cnrma_unet_join_abi_version(void) { return CNRMA_UNET_JOIN_ABI_VERSION; }

int cnrma_unet_join_supported(int B, int Cc, int Cf, int Xc, int Yc, int Zc) { return shape_ok(B, Cc, Cf, Xc, Yc, Zc) ? 1 : 0; }

size_t cnrma_unet_join_scratch_bytes(int B, int Cc, int Cf, int Xc, int Yc, int Zc) {
  return shape_ok(B, Cc, Cf, Xc, Yc, Zc) ? (size_t)B * Cf * Xc * Yc * Zc * 4 : 0;
}

int cnrma_unet_join_observed(const float* x, int B, int C, int X, int Y, int Z, unsigned char* observed, float* bound_x,
                             void* stream) {
  if (B < 1 || B > 65535 || C < 1 || X < 1 || Y < 1 || Z < 1 || x == nullptr || observed == nullptr) return CNRMA_UNET_JOIN_EINVAL;
  const int64_t lim = (int64_t)1 << 31;
  if (X >= lim / Y || (int64_t)X * Y >= lim / Z || (int64_t)X * Y * Z >= lim / ((int64_t)B * C)) return CNRMA_UNET_JOIN_EINVAL;
  hipStream_t st = as_stream(stream);
  if (bound_x != nullptr) {
    hipError_t err = cnrma_fill_bytes(bound_x, 0, (size_t)CNRMA_UNET_JOIN_BOUND_WORDS * 4, st);
    if (err != hipSuccess) return -(int)err;
  }
  const int N = X * Y * Z;
  hipLaunchKernelGGL(unetjoin_observed_kernel, dim3((unsigned)ceil_div(N, 256 * 4), (unsigned)B), dim3(256), 0, st, x, C, N, observed,
                     bound_x);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

int cnrma_unet_join_forward(const float* xc, const float* e, const float* w_up, const float* w_proj, const float* scale,
                            const float* shift, const unsigned char* observed, int step, int B, int Cc, int Cf, int Xc, int Yc,
                            int Zc, void* scratch, float* out, float* bound_out, void* stream) {
  if (!shape_ok(B, Cc, Cf, Xc, Yc, Zc) || xc == nullptr || e == nullptr || w_up == nullptr || w_proj == nullptr ||
      scratch == nullptr || out == nullptr || ((uintptr_t)scratch & 15) != 0 || (observed != nullptr && step < 1) ||
      (scale == nullptr) != (shift == nullptr))
    return CNRMA_UNET_JOIN_EINVAL;
  if (observed != nullptr && (int64_t)step * 2 * (Xc > Yc ? (Xc > Zc ? Xc : Zc) : (Yc > Zc ? Yc : Zc)) >= ((int64_t)1 << 31))
    return CNRMA_UNET_JOIN_EINVAL;           // the mask's dimensions are ints
  hipStream_t st = as_stream(stream);
  if (bound_out != nullptr) {
    hipError_t err = cnrma_fill_bytes(bound_out, 0, (size_t)CNRMA_UNET_JOIN_BOUND_WORDS * 4, st);
    if (err != hipSuccess) return -(int)err;
  }
  float* v = reinterpret_cast<float*>(scratch);
  const int Nc = Xc * Yc * Zc, nct = Cf / 32;
  hipLaunchKernelGGL(unetjoin_up_kernel, dim3((unsigned)ceil_div(Nc, WAVES * UP_VT * 32), (unsigned)nct, (unsigned)B), dim3(64 * WAVES),
                     (size_t)Cc * WPAD * 4, st, xc, w_up, Cc, Cf, Nc, v);
  CNRMA_LAUNCH_CHECK();
  const int64_t nbx = ceil_div(2 * Xc, TX), nby = ceil_div(2 * Yc, TY), nbz = ceil_div(2 * Zc, TZ);
  hipLaunchKernelGGL(unetjoin_fuse_kernel, dim3((unsigned)(nbx * nby * nbz * nct), 1, (unsigned)B), dim3(64 * WAVES),
                     (size_t)(32 * CHS > Cf * WPAD ? 32 * CHS : Cf * WPAD) * 4, st, v, e, w_proj, scale, shift, observed, step, Cf, Xc, Yc, Zc, nct, (int)nby,
                     (int)nbz, out, bound_out);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
