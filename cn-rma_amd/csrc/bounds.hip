// Bounds of the fusion volume on the device: exact order statistics of the back-projected depth pixels (reference:
// data_prepare/scannet/generate_tsdf.py:82-101 -- depth_to_world per frame, a concatenated cloud, a finite filter, a copy to the host
// and two np.quantile).  include/cnrma_prep.h (p1) holds the contract; the pinned behaviour is the reference ON THE CPU, bit for bit.
//
// No cloud is stored: a radix select over the order-preserving 32-bit key of the float, four passes of 8 bits, each of which
// recomputes the point from its depth pixel (4 bytes per pixel and pass).  A block walks tiles of 256 consecutive pixels of ONE view:
// lanes own consecutive pixels of a row (whole-line depth loads), Pinv[v] is block-uniform.  Pass 0 counts the kept pixels and the
// NaNs per axis and histograms the top digit per axis; a one-block kernel forms the four ranks per axis and picks bucket and residual
// rank of the 12 targets; passes 1..3 histogram the next digit of the values under each axis's active prefixes (targets that share a
// prefix share a histogram: the first of them leads); after the last digit the key IS the value.  Histograms are built in LDS with
// integer atomics and merged into global counters with integer atomics: the sums do not depend on the order.  No float atomics, no
// reciprocals, no fused operation that is not an explicit fmaf, nothing read back, no tuning state.
#include <math.h>

#include "../../include/cnrma_prep.h"
#include "common.h"

namespace {

constexpr int BOUNDS_BLOCK = 256;
constexpr int BOUNDS_MAX_BLOCKS = 2048;            // 256 CUs x 8 blocks: one sweep of the grid; more tiles than that are looped over
constexpr int BINS = 256;                          // 8-bit digits, 4 passes
// workspace, in 32-bit words: [0] n, [1..3] NaNs per axis, then per target (axis * 4 + quantile * 2 + (k, k1)) its prefix, its
// residual rank and the target whose histogram it reads in the next pass; then the histograms of pass 0 (3) and of passes 1..3 (12 each)
constexpr int WS_COUNTS = 0, WS_PREFIX = 4, WS_RANK = 16, WS_LEADER = 28, WS_HIST0 = 64;
constexpr int WS_HIST1 = WS_HIST0 + 3 * BINS;
constexpr int WS_WORDS = WS_HIST1 + 3 * 12 * BINS;

struct BoundsParams {
  int V, H, W;
  float max_depth;
  int64_t hw, tiles_per_view, tiles;
};

// order-preserving key: negative values bit-flipped, the others with the top bit set; -0.0 is +0.0, every NaN is the last key
__device__ __forceinline__ uint32_t key_of(float w) {
  if (w != w) return 0xFFFFFFFFu;
  if (w == 0.0f) w = 0.0f;
  const uint32_t u = __float_as_uint(w);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// PASS 0: counts + top digit per axis; PASS 1..3: digit PASS of the values whose first PASS digits equal an active prefix of their axis
template <int PASS>
__global__ __launch_bounds__(BOUNDS_BLOCK) void bounds_hist_kernel(BoundsParams p, const float* __restrict__ pinv,
                                                                   const float* __restrict__ depth,
                                                                   const uint32_t* __restrict__ state, uint32_t* __restrict__ counts,
                                                                   uint32_t* __restrict__ ghist) {
  constexpr int NH = PASS == 0 ? 3 : 12;
  __shared__ uint32_t hist[NH * BINS];
  __shared__ uint32_t cnt[4];
  for (int i = threadIdx.x; i < NH * BINS; i += BOUNDS_BLOCK) hist[i] = 0;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  uint32_t prefix[12];
  bool leads[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) {
    prefix[t] = PASS == 0 ? 0u : state[WS_PREFIX + t];                            // block-uniform
    leads[t] = PASS != 0 && state[WS_LEADER + t] == (uint32_t)t;
  }
  __syncthreads();

  uint32_t kept_here = 0;
  const uint32_t lane = threadIdx.x & 63u, tiles_per_view = (uint32_t)p.tiles_per_view, hw = (uint32_t)p.hw, W = (uint32_t)p.W;
  for (uint32_t tile = blockIdx.x; tile < (uint32_t)p.tiles; tile += gridDim.x) {    // tiles <= V H W < 2^31: 32-bit index arithmetic
    const uint32_t v = tile / tiles_per_view;
    const uint32_t i = (tile - v * tiles_per_view) * BOUNDS_BLOCK + threadIdx.x;     // pixel of view v
    if (i >= hw) continue;
    const float* __restrict__ M = pinv + (size_t)v * 16;                           // block-uniform address
    const uint32_t py = i / W, px = i - py * W;
    float d = depth[(size_t)v * hw + i];
    if (d > p.max_depth) d = 0.0f;                                                 // generate_tsdf.py:94
    const float p0 = (float)px, p1 = (float)py, p3 = 1.0f / d;                     // tsdf.py:92-96  an IEEE division
    float Q[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                                  // tsdf.py:99  inverse @ p, as the CPU's sgemm evaluates
      float acc = M[r * 4 + 0] * p0;                                               // it (oracle.rma_oracle.matmul_fma_chain)
      acc = fmaf(M[r * 4 + 1], p1, acc);
      acc = fmaf(M[r * 4 + 2], 1.0f, acc);
      acc = fmaf(M[r * 4 + 3], p3, acc);
      Q[r] = acc;
    }
    const float w0 = Q[0] / Q[3];                                                  // tsdf.py:100
    if (!(fabsf(w0) < INFINITY)) continue;                                         // generate_tsdf.py:97  kept iff x is finite
    const float w[3] = {w0, Q[1] / Q[3], Q[2] / Q[3]};
    if constexpr (PASS == 0) ++kept_here;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t key = key_of(w[a]);
      if constexpr (PASS == 0) {
        if (w[a] != w[a]) atomicAdd(&cnt[1 + a], 1u);
        // the coordinates of a scene share a few leading digits: the lanes of a wave that hold the same digit add once, together
        const uint32_t bin = key >> 24;
        for (bool pending = true; pending;) {
          const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
          const bool mine = bin == first;
          const uint64_t same = __ballot(mine);
          if (mine) {
            if ((uint32_t)(__ffsll((long long)same) - 1) == lane) atomicAdd(&hist[a * BINS + first], (uint32_t)__popcll(same));
            pending = false;
          }
        }
      } else {
        const uint32_t head = key >> (32 - 8 * PASS), digit = (key >> (24 - 8 * PASS)) & 0xFFu;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (leads[a * 4 + j] && head == prefix[a * 4 + j]) atomicAdd(&hist[(a * 4 + j) * BINS + digit], 1u);
      }
    }
  }
  if constexpr (PASS == 0) {
    if (kept_here != 0) atomicAdd(&cnt[0], kept_here);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NH * BINS; i += BOUNDS_BLOCK)
    if (hist[i] != 0) atomicAdd(&ghist[i], hist[i]);
  if constexpr (PASS == 0) {
    if (threadIdx.x < 4 && cnt[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]);
  }
}

// one block of four waves, three targets each (target t: axis t / 4, quantile (t / 2) % 2, k or k1): after pass `pass` a wave walks
// the histogram its target was counted in -- four bins per lane and a wave scan --, appends the digit that holds its rank to its prefix
// and keeps the rank inside that bucket.  Pass 0 first forms the ranks; pass 3 ends with the values.
__global__ __launch_bounds__(256) void bounds_select_kernel(int pass, float q_lo, float q_hi, uint32_t* __restrict__ ws,
                                                            float* __restrict__ out_values, int64_t* __restrict__ out_counts) {
  __shared__ uint32_t new_prefix[12];
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)ws[WS_COUNTS];
  if (pass == 0 && threadIdx.x < 4) out_counts[threadIdx.x] = (int64_t)ws[WS_COUNTS + threadIdx.x];
  if (n == 0) return;                                                               // block-uniform: nothing to select, values untouched
  for (int t = threadIdx.x >> 6; t < 12; t += 4) {                                  // wave-uniform
    const int a = t >> 2, j = t & 3;
    uint32_t rank, prefix;
    const uint32_t* hist;
    if (pass == 0) {
      // numpy's virtual index for a float32 sample and a Python-float q: (n - 1) * q in fp32; previous = floor, next = previous + 1 in
      // fp32; at or beyond n - 1 both are the last element
      const float last = (float)(n - 1), vi = last * ((j >> 1) ? q_hi : q_lo);
      int64_t k = n - 1, k1 = n - 1;
      if (!(vi >= last)) {
        const float f = floorf(vi);
        k = (int64_t)f;                                                             // vi < (float)(n - 1), so k <= n - 1
        k1 = (int64_t)(f + 1.0f);                                                   // an fp32 sum: it can round to k, or beyond n - 1
        k1 = k1 < n - 1 ? k1 : n - 1;
      }
      rank = (uint32_t)((j & 1) ? k1 : k);
      prefix = 0;
      hist = ws + WS_HIST0 + a * BINS;
    } else {
      rank = ws[WS_RANK + t];
      prefix = ws[WS_PREFIX + t];
      hist = ws + WS_HIST1 + ((pass - 1) * 12 + (int)ws[WS_LEADER + t]) * BINS;
    }
    const uint4 c = reinterpret_cast<const uint4*>(hist)[lane];                     // bins 4 lane .. 4 lane + 3 (16-byte aligned)
    const uint32_t mine = c.x + c.y + c.z + c.w;
    const uint32_t upto = (uint32_t)wave_incl_scan((int)mine), before = upto - mine; // totals stay below 2^31
    if (rank >= before && rank < upto) {                                            // rank < the histogram's total: exactly one lane
      uint32_t r = rank - before, b = 4u * (uint32_t)lane;
      if (r >= c.x) { r -= c.x; ++b;
        if (r >= c.y) { r -= c.y; ++b;
          if (r >= c.z) { r -= c.z; ++b; } } }
      prefix = (prefix << 8) | b;
      new_prefix[t] = prefix;
      ws[WS_RANK + t] = r;
      ws[WS_PREFIX + t] = prefix;
      if (pass == 3) out_values[(((j >> 1) * 3 + a) << 1) + (j & 1)] = value_of(prefix);
    }
  }
  __syncthreads();
  if (threadIdx.x < 12) {
    const int t = threadIdx.x;
    int lead = t;
    for (int u = (t & ~3); u < t; ++u)
      if (new_prefix[u] == new_prefix[t]) { lead = u; break; }
    ws[WS_LEADER + t] = (uint32_t)lead;
  }
}

}  // namespace

extern "C" int cnrma_prep_abi_version(void) { return CNRMA_PREP_ABI_VERSION; }

extern "C" size_t cnrma_prep_bounds_workspace_bytes(void) { return (size_t)WS_WORDS * 4; }

extern "C" int cnrma_prep_depth_bounds_f32(const float* pinv, const float* depth, int V, int H, int W, float max_depth, double q_lo,
                                           double q_hi, void* workspace, size_t workspace_bytes, float* out_values,
                                           int64_t* out_counts, void* stream) {
  if (V < 0 || H < 0 || W < 0) return CNRMA_PREP_EINVAL;
  const int64_t hw = (int64_t)H * W;
  if (hw >= ((int64_t)1 << 31) || (int64_t)V * hw >= ((int64_t)1 << 31)) return CNRMA_PREP_EINVAL;
  if (!(q_lo >= 0.0 && q_lo <= 1.0) || !(q_hi >= 0.0 && q_hi <= 1.0)) return CNRMA_PREP_EINVAL;
  if (workspace == nullptr || workspace_bytes < (size_t)WS_WORDS * 4 || ((uintptr_t)workspace & 15) != 0) return CNRMA_PREP_EINVAL;
  if (out_values == nullptr || out_counts == nullptr) return CNRMA_PREP_EINVAL;
  const int64_t total = (int64_t)V * hw;
  if (total != 0 && (pinv == nullptr || depth == nullptr)) return CNRMA_PREP_EINVAL;
  hipStream_t st = as_stream(stream);
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  hipError_t e = cnrma_fill_bytes(ws, 0, (size_t)WS_WORDS * 4, st);
  if (e != hipSuccess) return -(int)e;
  BoundsParams p{V, H, W, max_depth, hw, 0, 0};
  p.tiles_per_view = ceil_div(hw, BOUNDS_BLOCK);
  p.tiles = p.tiles_per_view * V;
  const dim3 grid((unsigned)(p.tiles < BOUNDS_MAX_BLOCKS ? p.tiles : BOUNDS_MAX_BLOCKS)), block(BOUNDS_BLOCK);
  const float ql = (float)q_lo, qh = (float)q_hi;
  for (int pass = 0; pass < 4; ++pass) {
    if (total != 0) {
      uint32_t* gh = ws + (pass == 0 ? WS_HIST0 : WS_HIST1 + (pass - 1) * 12 * BINS);
      if (pass == 0) hipLaunchKernelGGL(bounds_hist_kernel<0>, grid, block, 0, st, p, pinv, depth, ws, ws + WS_COUNTS, gh);
      else if (pass == 1) hipLaunchKernelGGL(bounds_hist_kernel<1>, grid, block, 0, st, p, pinv, depth, ws, ws + WS_COUNTS, gh);
      else if (pass == 2) hipLaunchKernelGGL(bounds_hist_kernel<2>, grid, block, 0, st, p, pinv, depth, ws, ws + WS_COUNTS, gh);
      else hipLaunchKernelGGL(bounds_hist_kernel<3>, grid, block, 0, st, p, pinv, depth, ws, ws + WS_COUNTS, gh);
      CNRMA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bounds_select_kernel, dim3(1), dim3(256), 0, st, pass, ql, qh, ws, out_values, out_counts);
    CNRMA_LAUNCH_CHECK();
    if (total == 0) break;                                                          // n = 0 is written; nothing to select
  }
  return 0;
}
