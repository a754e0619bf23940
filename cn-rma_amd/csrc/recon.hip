// The TSDF regression head on the device (include/cnrma_recon.h): one scale of AtlasTSDFHead -- 1x1x1 convolution, tanh, the
// sparsifying +-0.999 fill from the previous scale, the log-space L1 loss and the backward of all of it.
//   recon_head_forward_kernel     one lane per voxel: parent, near, then (near lanes only) C strided loads of x; writes tsdf
//   recon_head_loss_kernel        one workgroup per run of whole z-columns: column flags in LDS, then the terms; writes dloss and
//                                 one (fp64 sum, count) partial                          -> recon_head_loss_final_kernel
//   recon_head_backward_kernel    one wave per 512 voxels, 8 per lane: g_y in registers, then per channel the dx stores and the
//                                 fp64 dw partial of the wave                            -> recon_head_dw_final_kernel
// A voxel's x values lie V = X*Y*Z elements apart; consecutive lanes take consecutive voxels, so every load and store of a wave is
// one contiguous run.  No floating-point atomics anywhere: every sum has one fixed order.
#include <math.h>

#include "../../include/cnrma_recon.h"
#include "common.h"

namespace {

constexpr int RECON_BLOCK = 256;
constexpr int RECON_WAVES = RECON_BLOCK / 64;
constexpr int RECON_LOSS_CHUNK = 2048;      // voxels of whole columns per workgroup of the loss (one column when Z is larger)
constexpr int RECON_BWD_ITEMS = 8;          // voxels per lane of the backward
constexpr int RECON_BWD_WAVE = 64 * RECON_BWD_ITEMS;

static_assert(CNRMA_RECON_ELEM_F16 == CNRMA_ELEM_F16 && CNRMA_RECON_ELEM_BF16 == CNRMA_ELEM_BF16, "the 16-bit codes are cnrma.h's");

template <int ELEM> struct ReconElem;
template <> struct ReconElem<CNRMA_RECON_ELEM_F32> {
  using T = float;
  static __device__ __forceinline__ float load(const T* p) { return *p; }
  static __device__ __forceinline__ T round(float v) { return v; }
};
template <> struct ReconElem<CNRMA_RECON_ELEM_F16> {
  using T = uint16_t;
  static __device__ __forceinline__ float load(const T* p) { return elem16_to_f32<CNRMA_ELEM_F16>(*p); }
  // nearest even, of the fp32 value as it stands: the empty statement keeps the compiler from folding the caller's multiplication
  // into the conversion (v_fma_mixlo_f16 rounds the exact product instead, and dx would differ from the fp32 kernel's rounded)
  static __device__ __forceinline__ T round(float v) {
    asm volatile("" : "+v"(v));
    return __builtin_bit_cast(uint16_t, (_Float16)v);
  }
};
template <> struct ReconElem<CNRMA_RECON_ELEM_BF16> {
  using T = uint16_t;
  static __device__ __forceinline__ float load(const T* p) { return elem16_to_f32<CNRMA_ELEM_BF16>(*p); }
  static __device__ __forceinline__ T round(float v) {                                                         // nearest even
    uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
  }
};

struct ReconGrid {
  int X, Y, Z;
  int64_t V, N;               // voxels per batch element, B * V
  const float* prev;          // NULL at the first scale
  float threshold;
};

// the parent's value of flat voxel n = b * V + v (nearest x2 up-sampling: every index halves); g.prev is not NULL
__device__ __forceinline__ float recon_parent(const ReconGrid& g, int64_t n) {
  const int64_t b = n / g.V, v = n - b * g.V;
  const int64_t r = v / g.Z;
  const int iz = (int)(v - r * g.Z), ix = (int)(r / g.Y), iy = (int)(r - (int64_t)ix * g.Y);
  return g.prev[((b * (g.X >> 1) + (ix >> 1)) * (g.Y >> 1) + (iy >> 1)) * (g.Z >> 1) + (iz >> 1)];
}

__device__ __forceinline__ bool recon_near(const ReconGrid& g, int64_t n, float* u) {
  if (g.prev == nullptr) { *u = 0.0f; return true; }
  *u = recon_parent(g, n);
  return fabsf(*u) < g.threshold;
}

__device__ __forceinline__ float recon_lt(float v) { return copysignf(log1pf(fabsf(v)), v); }

__device__ __forceinline__ double recon_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}
__device__ __forceinline__ long long recon_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// (sum, count) of a workgroup: lanes by the shuffle tree, waves in order; the result is valid in thread 0
__device__ __forceinline__ void recon_block_sum(double* s, long long* c) {
  __shared__ double ws[RECON_WAVES];
  __shared__ long long wc[RECON_WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double s1 = recon_wave_sum(*s);
  const long long c1 = recon_wave_sum(*c);
  if (lane == 0) { ws[wid] = s1; wc[wid] = c1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double st = ws[0];
    long long ct = wc[0];
    for (int i = 1; i < RECON_WAVES; ++i) { st += ws[i]; ct += wc[i]; }
    *s = st;
    *c = ct;
  }
}

// FORWARD.  The channel loop sits under `if (near)`: a wave without a near lane branches over it and issues no load of x
template <int ELEM>
__global__ __launch_bounds__(RECON_BLOCK) void recon_head_forward_kernel(const typename ReconElem<ELEM>::T* __restrict__ x,
                                                                        const float* __restrict__ w, ReconGrid g, int C,
                                                                        float label_smoothing, float* __restrict__ tsdf) {
  using E = ReconElem<ELEM>;
  const int64_t n = (int64_t)blockIdx.x * RECON_BLOCK + threadIdx.x;
  if (n >= g.N) return;
  float u;
  const bool near = recon_near(g, n, &u);
  float out;
  if (near) {
    const int64_t b = n / g.V;
    const typename E::T* px = x + b * C * g.V + (n - b * g.V);
    float y = 0.0f;
    int c = 0;
    for (; c + 4 <= C; c += 4) {               // four loads leave together; the sum keeps its ascending order
      const float a0 = E::load(px + (int64_t)c * g.V), a1 = E::load(px + (int64_t)(c + 1) * g.V);
      const float a2 = E::load(px + (int64_t)(c + 2) * g.V), a3 = E::load(px + (int64_t)(c + 3) * g.V);
      y = fmaf(a0, w[c], y);
      y = fmaf(a1, w[c + 1], y);
      y = fmaf(a2, w[c + 2], y);
      y = fmaf(a3, w[c + 3], y);
    }
    for (; c < C; ++c) y = fmaf(E::load(px + (int64_t)c * g.V), w[c], y);
    out = tanhf(y) * label_smoothing;
  } else {
    out = (float)((u > 0.0f) - (u < 0.0f)) * 0.999f;
  }
  tsdf[n] = out;
}

// LOSS.  Workgroup j owns the columns [j * cols, (j + 1) * cols) of the B*X*Y columns, i.e. one contiguous run of voxels; a
// column's flag (all of its targets are exactly 1) is cleared in LDS by whoever finds another value (same value from every writer)
__global__ __launch_bounds__(RECON_BLOCK) void recon_head_loss_kernel(const float* __restrict__ tsdf, const float* __restrict__ trgt,
                                                                     ReconGrid g, int64_t n_cols, int cols,
                                                                     float* __restrict__ dloss, double* __restrict__ part_sum,
                                                                     long long* __restrict__ part_cnt) {
  __shared__ int all_one[RECON_LOSS_CHUNK];
  const int tid = threadIdx.x;
  const int64_t col0 = (int64_t)blockIdx.x * cols;
  const int n_col = n_cols - col0 < cols ? (int)(n_cols - col0) : cols;
  const int64_t base = col0 * g.Z;
  const int len = n_col * g.Z;
  for (int i = tid; i < n_col; i += RECON_BLOCK) all_one[i] = 1;
  __syncthreads();
  for (int i = tid; i < len; i += RECON_BLOCK)
    if (!(trgt[base + i] == 1.0f)) all_one[i / g.Z] = 0;
  __syncthreads();
  double s = 0.0;
  long long cnt = 0;
  for (int i = tid; i < len; i += RECON_BLOCK) {
    const int64_t n = base + i;
    const float t = trgt[n];
    bool use = (t < 1.0f) || all_one[i / g.Z] != 0;
    float u;
    use = use && recon_near(g, n, &u);
    float d = 0.0f;
    if (use) {
      const float p = tsdf[n];
      s += (double)fabsf(recon_lt(p) - recon_lt(t));
      cnt += 1;
      d = p != 0.0f ? (float)((p > t) - (p < t)) / (1.0f + fabsf(p)) : 0.0f;
    }
    if (dloss != nullptr) dloss[n] = d;
  }
  recon_block_sum(&s, &cnt);
  if (tid == 0) { part_sum[blockIdx.x] = s; part_cnt[blockIdx.x] = cnt; }
}

__global__ __launch_bounds__(RECON_BLOCK) void recon_head_loss_final_kernel(const double* __restrict__ part_sum,
                                                                           const long long* __restrict__ part_cnt, int n_parts,
                                                                           int first_scale, float* __restrict__ loss,
                                                                           long long* __restrict__ count) {
  double s = 0.0;
  long long cnt = 0;
  for (int i = threadIdx.x; i < n_parts; i += RECON_BLOCK) { s += part_sum[i]; cnt += part_cnt[i]; }
  recon_block_sum(&s, &cnt);
  if (threadIdx.x == 0) {
    count[0] = cnt;
    loss[0] = cnt > 0 ? (float)(s / (double)cnt) : (first_scale ? __builtin_nanf("") : 0.0f);
  }
}

// BACKWARD.  Wave `gw` owns the voxels [gw * 512, gw * 512 + 512): lane l takes gw * 512 + k * 64 + l, k = 0 .. 7
template <int ELEM>
__global__ __launch_bounds__(RECON_BLOCK) void recon_head_backward_kernel(
    const typename ReconElem<ELEM>::T* __restrict__ x, const float* __restrict__ w, ReconGrid g, int C, float label_smoothing,
    const float* __restrict__ tsdf, const float* __restrict__ grad_tsdf, const float* __restrict__ dloss,
    const float* __restrict__ grad_loss, const long long* __restrict__ count, int n_parts,
    typename ReconElem<ELEM>::T* __restrict__ dx, double* __restrict__ part) {
  using E = ReconElem<ELEM>;
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * RECON_WAVES + (threadIdx.x >> 6);
  if (gw >= n_parts) return;
  float scale = 0.0f;
  if (dloss != nullptr) {
    const long long cn = count[0];
    if (cn > 0) scale = grad_loss[0] / (float)cn;
  }
  float gy[RECON_BWD_ITEMS];
  int64_t off[RECON_BWD_ITEMS];             // of the voxel's channel 0 in x / dx; -1: past the end
#pragma unroll
  for (int k = 0; k < RECON_BWD_ITEMS; ++k) {
    const int64_t n = (int64_t)gw * RECON_BWD_WAVE + k * 64 + lane;
    gy[k] = 0.0f;
    off[k] = -1;
    if (n < g.N) {
      const int64_t b = n / g.V;
      off[k] = b * C * g.V + (n - b * g.V);
      float u;
      if (recon_near(g, n, &u)) {
        float gv = grad_tsdf != nullptr ? grad_tsdf[n] : 0.0f;
        if (dloss != nullptr) gv += scale * dloss[n];
        if (gv != 0.0f) {
          const float r = label_smoothing != 0.0f ? tsdf[n] / label_smoothing : 0.0f;
          gy[k] = gv * (label_smoothing * (1.0f - r * r));
        }
      }
    }
  }
  for (int c = 0; c < C; ++c) {
    const float wc = w[c];
    const int64_t co = (int64_t)c * g.V;
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < RECON_BWD_ITEMS; ++k) {
      if (off[k] < 0) continue;
      if (dx != nullptr) dx[off[k] + co] = E::round(gy[k] * wc);
      if (part != nullptr && gy[k] != 0.0f) p = fma((double)gy[k], (double)E::load(x + off[k] + co), p);
    }
    if (part != nullptr) {
      p = recon_wave_sum(p);
      if (lane == 0) part[(int64_t)c * n_parts + gw] = p;
    }
  }
}

__global__ __launch_bounds__(RECON_BLOCK) void recon_head_dw_final_kernel(const double* __restrict__ part, int n_parts,
                                                                         float* __restrict__ dw) {
  const double* row = part + (int64_t)blockIdx.x * n_parts;
  double s = 0.0;
  long long unused = 0;
  for (int i = threadIdx.x; i < n_parts; i += RECON_BLOCK) s += row[i];
  recon_block_sum(&s, &unused);
  if (threadIdx.x == 0) dw[blockIdx.x] = (float)s;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

struct ReconShape {
  int64_t V, N, n_cols;
  int cols;                    // columns per workgroup of the loss
  int64_t loss_parts, bwd_parts;
};

bool recon_shape(int B, int C, int X, int Y, int Z, ReconShape* s) {
  if (B < 1 || C < 1 || X < 1 || Y < 1 || Z < 1) return false;
  s->V = (int64_t)X * Y;
  if (s->V >= ((int64_t)1 << 31)) return false;
  s->V *= Z;
  if (s->V >= ((int64_t)1 << 31)) return false;
  s->N = s->V * B;
  if (s->N >= ((int64_t)1 << 31)) return false;
  s->n_cols = (int64_t)B * X * Y;
  s->cols = RECON_LOSS_CHUNK / Z < 1 ? 1 : RECON_LOSS_CHUNK / Z;
  s->loss_parts = ceil_div(s->n_cols, s->cols);
  s->bwd_parts = ceil_div(s->N, RECON_BWD_WAVE);
  return true;
}

bool recon_prev_ok(const float* prev, int PX, int PY, int PZ, int X, int Y, int Z) {
  if (prev == nullptr) return PX == 0 && PY == 0 && PZ == 0;
  return PX >= 1 && PY >= 1 && PZ >= 1 && X == 2 * PX && Y == 2 * PY && Z == 2 * PZ;
}

size_t recon_align16(size_t n) { return (n + 15) & ~(size_t)15; }
size_t recon_loss_bytes(const ReconShape& s) { return recon_align16((size_t)s.loss_parts * 8) + recon_align16((size_t)s.loss_parts * 8); }
size_t recon_bwd_bytes(const ReconShape& s, int C) { return recon_align16((size_t)s.bwd_parts * (size_t)C * 8); }

}  // namespace

extern "C" {

int cnrma_recon_abi_version(void) { return CNRMA_RECON_ABI_VERSION; }

size_t cnrma_recon_head_workspace_bytes(int B, int C, int X, int Y, int Z) {
  ReconShape s;
  if (!recon_shape(B, C, X, Y, Z, &s)) return 0;
  const size_t a = recon_loss_bytes(s), b = recon_bwd_bytes(s, C);
  return a > b ? a : b;
}

int cnrma_recon_head_forward(const void* x, int elem, const float* w, const float* prev, int PX, int PY, int PZ, float threshold,
                             float label_smoothing, int B, int C, int X, int Y, int Z, float* tsdf, void* stream) {
  ReconShape s;
  if (!recon_shape(B, C, X, Y, Z, &s) || !recon_prev_ok(prev, PX, PY, PZ, X, Y, Z)) return CNRMA_RECON_EINVAL;
  if (x == nullptr || w == nullptr || tsdf == nullptr) return CNRMA_RECON_EINVAL;
  if (elem != CNRMA_RECON_ELEM_F32 && elem != CNRMA_RECON_ELEM_F16 && elem != CNRMA_RECON_ELEM_BF16) return CNRMA_RECON_EINVAL;
  const ReconGrid g{X, Y, Z, s.V, s.N, prev, threshold};
  const dim3 grid((unsigned)ceil_div(s.N, RECON_BLOCK)), block(RECON_BLOCK);
  if (elem == CNRMA_RECON_ELEM_F32)
    hipLaunchKernelGGL(recon_head_forward_kernel<CNRMA_RECON_ELEM_F32>, grid, block, 0, as_stream(stream),
                       static_cast<const float*>(x), w, g, C, label_smoothing, tsdf);
  else if (elem == CNRMA_RECON_ELEM_F16)
    hipLaunchKernelGGL(recon_head_forward_kernel<CNRMA_RECON_ELEM_F16>, grid, block, 0, as_stream(stream),
                       static_cast<const uint16_t*>(x), w, g, C, label_smoothing, tsdf);
  else
    hipLaunchKernelGGL(recon_head_forward_kernel<CNRMA_RECON_ELEM_BF16>, grid, block, 0, as_stream(stream),
                       static_cast<const uint16_t*>(x), w, g, C, label_smoothing, tsdf);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

int cnrma_recon_head_loss_f32(const float* tsdf, const float* prev, int PX, int PY, int PZ, float threshold, const float* trgt,
                              int B, int X, int Y, int Z, void* workspace, size_t workspace_bytes, float* dloss, float* loss,
                              int64_t* count, void* stream) {
  ReconShape s;
  if (!recon_shape(B, 1, X, Y, Z, &s) || !recon_prev_ok(prev, PX, PY, PZ, X, Y, Z)) return CNRMA_RECON_EINVAL;
  if (tsdf == nullptr || trgt == nullptr || loss == nullptr || count == nullptr || workspace == nullptr) return CNRMA_RECON_EINVAL;
  if (workspace_bytes < recon_loss_bytes(s) || ((uintptr_t)workspace & 15) != 0) return CNRMA_RECON_EINVAL;
  double* part_sum = static_cast<double*>(workspace);
  long long* part_cnt = reinterpret_cast<long long*>(static_cast<char*>(workspace) + recon_align16((size_t)s.loss_parts * 8));
  const ReconGrid g{X, Y, Z, s.V, s.N, prev, threshold};
  hipLaunchKernelGGL(recon_head_loss_kernel, dim3((unsigned)s.loss_parts), dim3(RECON_BLOCK), 0, as_stream(stream), tsdf, trgt, g,
                     s.n_cols, s.cols, dloss, part_sum, part_cnt);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(recon_head_loss_final_kernel, dim3(1), dim3(RECON_BLOCK), 0, as_stream(stream), part_sum, part_cnt,
                     (int)s.loss_parts, prev == nullptr ? 1 : 0, loss, reinterpret_cast<long long*>(count));
  CNRMA_LAUNCH_CHECK();
  return 0;
}

int cnrma_recon_head_backward(const void* x, int elem, const float* w, const float* prev, int PX, int PY, int PZ, float threshold,
                              float label_smoothing, const float* tsdf, const float* grad_tsdf, const float* dloss,
                              const float* grad_loss, const int64_t* count, int B, int C, int X, int Y, int Z, void* workspace,
                              size_t workspace_bytes, void* dx, float* dw, void* stream) {
  ReconShape s;
  if (!recon_shape(B, C, X, Y, Z, &s) || !recon_prev_ok(prev, PX, PY, PZ, X, Y, Z)) return CNRMA_RECON_EINVAL;
  if (w == nullptr || tsdf == nullptr || (dw != nullptr && x == nullptr)) return CNRMA_RECON_EINVAL;
  if (dloss != nullptr && (grad_loss == nullptr || count == nullptr)) return CNRMA_RECON_EINVAL;
  if (elem != CNRMA_RECON_ELEM_F32 && elem != CNRMA_RECON_ELEM_F16 && elem != CNRMA_RECON_ELEM_BF16) return CNRMA_RECON_EINVAL;
  if (dw != nullptr && (workspace == nullptr || workspace_bytes < recon_bwd_bytes(s, C) || ((uintptr_t)workspace & 15) != 0))
    return CNRMA_RECON_EINVAL;
  if (dx == nullptr && dw == nullptr) return 0;
  double* part = dw != nullptr ? static_cast<double*>(workspace) : nullptr;
  const long long* cnt = reinterpret_cast<const long long*>(count);
  const ReconGrid g{X, Y, Z, s.V, s.N, prev, threshold};
  const dim3 grid((unsigned)ceil_div(s.bwd_parts, RECON_WAVES)), block(RECON_BLOCK);
  const int n_parts = (int)s.bwd_parts;
  if (elem == CNRMA_RECON_ELEM_F32)
    hipLaunchKernelGGL(recon_head_backward_kernel<CNRMA_RECON_ELEM_F32>, grid, block, 0, as_stream(stream),
                       static_cast<const float*>(x), w, g, C, label_smoothing, tsdf, grad_tsdf, dloss, grad_loss, cnt, n_parts,
                       static_cast<float*>(dx), part);
  else if (elem == CNRMA_RECON_ELEM_F16)
    hipLaunchKernelGGL(recon_head_backward_kernel<CNRMA_RECON_ELEM_F16>, grid, block, 0, as_stream(stream),
                       static_cast<const uint16_t*>(x), w, g, C, label_smoothing, tsdf, grad_tsdf, dloss, grad_loss, cnt, n_parts,
                       static_cast<uint16_t*>(dx), part);
  else
    hipLaunchKernelGGL(recon_head_backward_kernel<CNRMA_RECON_ELEM_BF16>, grid, block, 0, as_stream(stream),
                       static_cast<const uint16_t*>(x), w, g, C, label_smoothing, tsdf, grad_tsdf, dloss, grad_loss, cnt, n_parts,
                       static_cast<uint16_t*>(dx), part);
  CNRMA_LAUNCH_CHECK();
  if (dw != nullptr) {
    hipLaunchKernelGGL(recon_head_dw_final_kernel, dim3((unsigned)C), dim3(RECON_BLOCK), 0, as_stream(stream), part, n_parts, dw);
    CNRMA_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
