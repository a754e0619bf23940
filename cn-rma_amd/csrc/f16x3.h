// f16x3 operand arithmetic and the magnitude-bound convention, shared by sparse.hip and unet.hip (moved verbatim from sparse.hip).
#pragma once
#include "common.h"

// ---- f16x3: a * 2^s = h + m with h, m fp16 (round to nearest): |a 2^s - h - m| <= 2^-22 |a 2^s|; the products hh, hm, mh
// are exact in fp32, the dropped mm term is <= 2^-22 |ab|.  The power-of-two scale (from an upper bound of the
// tensor's magnitude) keeps the largest operand at 2^13..2^14: no overflow, and every element down to 2^-17 of the
// largest keeps its 22 bits before m runs into fp16 subnormals.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float f16_scale_for(float amax) {
  if (!(amax > 0.0f) || !(amax < 3.0e38f)) return 1.0f;
  int e;
  (void)frexpf(amax, &e);                                  // amax < 2^e
  int sh = 14 - e;
  sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
  return ldexpf(1.0f, sh);
}

__device__ __forceinline__ void split2_f16(float x, uint16_t& h, uint16_t& m) {
  const _Float16 hh = (_Float16)x;
  const float r = x - (float)hh;                            // exact
  const _Float16 mm = (_Float16)r;
  h = __builtin_bit_cast(uint16_t, hh);
  m = __builtin_bit_cast(uint16_t, mm);
}

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// (v * scale) -> fp16 pairs h, m in packed arithmetic: v_pk_mul_f32, v_cvt_pk_f16_f32, v_pk_add_f32 (3 VALU per value)
__device__ __forceinline__ void split2(const float4& v, float scale, uint2& h, uint2& m) {
  f32x2_t a = {v.x, v.y}, b = {v.z, v.w};
  a *= scale; b *= scale;
  const f16x2_t ha = __builtin_convertvector(a, f16x2_t), hb = __builtin_convertvector(b, f16x2_t);
  const f32x2_t ra = a - __builtin_convertvector(ha, f32x2_t), rb = b - __builtin_convertvector(hb, f32x2_t);   // exact
  const f16x2_t ma = __builtin_convertvector(ra, f16x2_t), mb = __builtin_convertvector(rb, f16x2_t);
  h = make_uint2(__builtin_bit_cast(uint32_t, ha), __builtin_bit_cast(uint32_t, hb));
  m = make_uint2(__builtin_bit_cast(uint32_t, ma), __builtin_bit_cast(uint32_t, mb));
}

// A tensor's magnitude bound lives in AMAX_SLOTS words, one per 64-byte line: a block publishes ONE candidate (wave
// shuffle + LDS), into the slot its block index hashes to, and only when it beats the value currently visible (the
// maximum is monotone, so a stale read only costs a redundant atomic).  Thousands of same-address atomics per launch
// serialise at the memory side (measured: +1.1 ms per scene with one atomic per wave on a single word).
constexpr int AMAX_SLOTS = 64, AMAX_STRIDE = 16;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ float read_amax(const float* slots) {            // every lane returns the bound
  return wave_max(slots[(threadIdx.x & 63) * AMAX_STRIDE]);
}

// one thread hands in its block's candidate m >= 0 (uint order == float order)
__device__ __forceinline__ void amax_publish_candidate(float* slots, float m) {
  const unsigned slot = (blockIdx.x + 7u * blockIdx.y + 13u * blockIdx.z) & (AMAX_SLOTS - 1);
  unsigned* d = reinterpret_cast<unsigned*>(slots + slot * AMAX_STRIDE);
  const unsigned bits = __float_as_uint(m);
  if (bits > __hip_atomic_load(d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(d, bits);
}

// v >= 0; blockDim.x == 64 * WAVES, every thread of the block calls it; sh: WAVES floats of LDS
template <int WAVES = 4>
__device__ __forceinline__ void block_amax_publish(float* slots, float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    // by pairs, not in sequence: the order is free (a maximum of non-negative values), and this one keeps the instruction
    // streams of the 256-thread callers, the sparse family's kernels, what they were
    float m = WAVES > 1 ? fmaxf(sh[0], sh[1]) : sh[0];
#pragma unroll
    for (int w = 2; w < WAVES; w += 2) m = fmaxf(m, w + 1 < WAVES ? fmaxf(sh[w], sh[w + 1]) : sh[w]);
    amax_publish_candidate(slots, m);
  }
}
