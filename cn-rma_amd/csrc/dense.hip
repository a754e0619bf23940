// Dense unprojection + accumulate + mean in ONE pass over the voxel grid.
//
// The reference makes V full passes: zero-fill + scatter a C x G volume per view, add it to a running sum,
// and finally divides by the view count (ray_marching.py:21-69, :220-257) -- 15 GB of writes per scene at the
// ScanNet shape.  Here each lane owns one voxel, loops over the V views with the accumulators in registers and
// writes the mean volume exactly once (compulsory traffic: read the feature planes, write C x G floats).
//
// Lane -> voxel mapping: linear index with z fastest, so the stores of one channel are coalesced; the gathers hit
// channels-last pixels (one 128-B line per pixel at C = 32).
// Bit-exactness: world = fl(fl(i*vs)+o); cam = fma chain (MKL bmm); px,py = rint(cam0/cam2) (IEEE division);
// sum in view order; mean = sum / (float)count.  Compiled with -ffp-contract=off.
#include "common.h"


namespace {

static __device__ __forceinline__ int64_t ceil_div_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct DenseParams {
  int V, C, H, W, X, Y, Z;
  float vs, ox, oy, oz;
};

__device__ __forceinline__ void voxel_world(const DenseParams& p, int64_t g, float* wx, float* wy, float* wz) {
  int x, y, z;
  if (((uint64_t)g >> 32) == 0) {                // 32-bit divisions wherever the index allows them: a quarter of the 64-bit ones' instructions
    const unsigned g32 = (unsigned)g, t = g32 / (unsigned)p.Z;
    z = (int)(g32 - t * (unsigned)p.Z);
    x = (int)(t / (unsigned)p.Y);
    y = (int)(t - (unsigned)x * (unsigned)p.Y);
  } else {
    z = (int)(g % p.Z);
    const int64_t t = g / p.Z;
    y = (int)(t % p.Y);
    x = (int)(t / p.Y);
  }
  *wx = (float)x * p.vs + p.ox;  // ray_marching.py:48  (two roundings)
  *wy = (float)y * p.vs + p.oy;
  *wz = (float)z * p.vs + p.oz;
}

// Brick order of the voxels (cooperative kernel).  Voxels that share a pixel lie on one camera ray, 8-64 voxels apart;
// a gathered pixel line is re-used only if two of them are processed by the SAME XCD (private 4 MB L2) at about the same
// time.  With the plain z-fastest order the voxels in flight on an XCD are a pile of thin vertical columns that a ray
// crosses once (TCC hit rate 22 %).  Here the grid is cut into bricks of st x st columns x zt layers (default 16 x 16 x 32
// = 8192 voxels = 32 workgroups), z fastest inside a column, columns in tt x tt tiles; every brick is a chunk that one XCD
// group owns (chunks c, c + 8, ... as before), so the ~8 bricks an XCD has in flight are compact 0.64 x 0.64 x 1.28 m
// boxes in which a ray meets several of its voxels.  Measured at the north-star shape (scripts/dense_ab.py, results
// bit-identical): 13.3 -> 10.7 ms; 64 x 64 x 16 slabs 12.8, 32 x 32 x 16 11.5, 16 x 16 x 64 10.8, 8 x 8 x 32 11.5,
// 128 x 128 x 16 19.0 ms.  A lane of the product kernel stores runs of 4 consecutive z (group_src_lane() below): whole 128-byte
// lines per store instruction where zi % 4 == 0 and the grid allows it.
struct SlabOrder {
  int on, nsx, nsy, nsz, zt, st, tt, zi, nt, own, stagger, groups;  // zt: z-layers per brick, st: brick side, tt: tile side (columns), zi: inner z run
  // p2: st, zt, tt, zi are powers of two and every block index fits 31 bits (the shipped schedule): blocks and threads are
  // decoded with 32-bit shifts and masks (block_decode(), remap_block()).  lcb = log2(blocks per brick), lzi = log2(zi),
  // ltt = log2(tt), lzo = log2(zt / zi), ltpr = log2(st / tt)
  int p2, lcb, lzi, ltt, lzo, ltpr;
};

__device__ __forceinline__ bool slab_decode(const DenseParams& p, const SlabOrder& o, int64_t gv, int* x, int* y, int* z) {
  const int64_t per = (int64_t)o.st * o.st * o.zt;
  const int64_t sv = gv / per;
  const int r = (int)(gv - sv * per);
  if (sv >= (int64_t)o.nsx * o.nsy * o.nsz) return false;
  const int sy = (int)(sv % o.nsy), sx = (int)((sv / o.nsy) % o.nsx), sz = (int)(sv / ((int64_t)o.nsy * o.nsx));
  // order inside a brick: [tile of tt x tt columns][outer z][column in tile][inner z run of zi]
  const int tcols = o.tt * o.tt, zo_n = o.zt / o.zi;
  const int zin = r % o.zi, q = r / o.zi;
  const int in = q % tcols, q2 = q / tcols;
  const int zo = q2 % zo_n, tile = q2 / zo_n;
  const int zl = zo * o.zi + zin;
  const int tpr = o.st / o.tt;
  *x = sx * o.st + (tile / tpr) * o.tt + in / o.tt;
  *y = sy * o.st + (tile % tpr) * o.tt + in % o.tt;
  *z = sz * o.zt + zl;
  return *x < p.X && *y < p.Y && *z < p.Z;
}

// slab_decode() of thread `tid` of logical block `lb` (voxel lb * 256 + tid).  With o.p2 the same (x, y, z) comes from 32-bit
// shifts and masks and two 32-bit divisions by the brick counts -- slab_decode()'s 64-bit divisions were most of the ~2200
// instructions a wave ran before its view loop, in every channel sweep.
__device__ __forceinline__ bool block_decode(const DenseParams& p, const SlabOrder& o, int64_t lb, int tid, int* x, int* y, int* z) {
  if (!o.p2) return slab_decode(p, o, lb * 256 + tid, x, y, z);
  const unsigned b = (unsigned)lb;
  const unsigned sv = b >> o.lcb;
  if (sv >= (unsigned)(o.nsx * o.nsy * o.nsz)) return false;
  const unsigned r = ((b & ((1u << o.lcb) - 1u)) << 8) | (unsigned)tid;
  const unsigned t = sv / (unsigned)o.nsy, sy = sv - t * (unsigned)o.nsy;
  const unsigned sz = t / (unsigned)o.nsx, sx = t - sz * (unsigned)o.nsx;
  const unsigned zin = r & (unsigned)(o.zi - 1), q = r >> o.lzi;
  const unsigned in = q & ((1u << (2 * o.ltt)) - 1u), q2 = q >> (2 * o.ltt);
  const unsigned zo = q2 & ((1u << o.lzo) - 1u), tile = q2 >> o.lzo;
  *x = (int)(sx * o.st + ((tile >> o.ltpr) << o.ltt) + (in >> o.ltt));
  *y = (int)(sy * o.st + ((tile & ((1u << o.ltpr) - 1u)) << o.ltt) + (in & (unsigned)(o.tt - 1)));
  *z = (int)(sz * o.zt + ((zo << o.lzi) | zin));
  return *x < p.X && *y < p.Y && *z < p.Z;
}

// Launch block -> logical block of the free-running grid: chunk c of `chunk_blocks` blocks belongs to XCD group c % 8 (launch
// blocks are dealt to the XCDs round-robin).  chunk_blocks <= 0: identity.  o.p2: chunk_blocks == 1 << o.lcb.
__device__ __forceinline__ int64_t remap_block(unsigned b, int chunk_blocks, const SlabOrder& o) {
  if (chunk_blocks <= 0) return b;
  if (o.p2) {
    const unsigned k = b >> 3;
    return (((b & 7u) + 8u * (k >> o.lcb)) << o.lcb) | (k & ((1u << o.lcb) - 1u));
  }
  const int64_t grp = b & 7, k = b >> 3;
  return (grp + 8 * (k / chunk_blocks)) * chunk_blocks + k % chunk_blocks;
}

// Lattice assignment of a brick's z-columns to its workgroups (lockstep schedule; zt == 32, st % 8 == 0): workgroup w of
// the st*st/8 takes 8 whole columns on a (2 x 4) lattice with pitch (st/2, st/4) -- column j at
// (w / (st/4) + (st/2) * (j / 4),  w % (st/4) + (st/4) * (j % 4)) --, so every workgroup samples the whole brick and meets
// each view's frustum boundary in the same proportion as its neighbours: equal work per view, the precondition for staying in
// phase.  A wave still owns 2 columns x 32 consecutive z (full 128-byte store runs per channel plane).
__device__ __forceinline__ bool lattice_decode(const DenseParams& p, const SlabOrder& o, int64_t lb, int tid, int* x, int* y, int* z) {
  const int cb = o.st * o.st / 8;
  const int64_t sv = lb / cb;
  if (sv >= (int64_t)o.nsx * o.nsy * o.nsz) return false;
  const int w = (int)(lb - sv * cb), j = tid >> 5, q4 = o.st / 4;
  const int sy = (int)(sv % o.nsy), sx = (int)((sv / o.nsy) % o.nsx), sz = (int)(sv / ((int64_t)o.nsy * o.nsx));
  *x = sx * o.st + w / q4 + (o.st / 2) * (j >> 2);
  *y = sy * o.st + w % q4 + q4 * (j & 3);
  *z = sz * 32 + (tid & 31);
  return *x < p.X && *y < p.Y && *z < p.Z;
}

// project one voxel into one view: returns validity, pixel in (*px,*py) (ray_marching.py:51-58)
__device__ __forceinline__ bool project(const float* __restrict__ P, float wx, float wy, float wz, int H, int W,
                                        float* rx, float* ry) {
  float cam[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float acc = P[r * 4 + 0] * wx;
    acc = fmaf(P[r * 4 + 1], wy, acc);
    acc = fmaf(P[r * 4 + 2], wz, acc);
    acc = fmaf(P[r * 4 + 3], 1.0f, acc);
    cam[r] = acc;
  }
  *rx = rintf(cam[0] / cam[2]);
  *ry = rintf(cam[1] / cam[2]);
  // comparisons in float are equivalent to the reference's int64 ones: NaN / out-of-range casts land on
  // INT64_MIN there (negative -> invalid), and are rejected here as well
  return (*rx >= 0.0f) && (*ry >= 0.0f) && (*rx < (float)W) && (*ry < (float)H) && (cam[2] > 0.0f);
}

// CT channels per lane kept in registers; grid.y walks channel chunks
template <int CT>
__global__ __launch_bounds__(256) void backproject_accum_kernel(DenseParams p, const float* __restrict__ feat,
                                                                const float* __restrict__ proj,
                                                                float* __restrict__ volume,
                                                                int32_t* __restrict__ count) {
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int c0 = blockIdx.y * CT;
  float wx, wy, wz;
  voxel_world(p, g, &wx, &wy, &wz);
  float acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0.0f;
  int cnt = 0;
  const int64_t plane = (int64_t)p.H * p.W * p.C;
  for (int v = 0; v < p.V; ++v) {
    float rx, ry;
    if (!project(proj + v * 12, wx, wy, wz, p.H, p.W, &rx, &ry)) continue;
    ++cnt;
    const float* f = feat + v * plane + ((int64_t)(int)ry * p.W + (int)rx) * p.C + c0;
    if constexpr (CT % 4 == 0) {
#pragma unroll
      for (int c = 0; c < CT; c += 4) {
        float4 q = *reinterpret_cast<const float4*>(f + c);
        acc[c] += q.x; acc[c + 1] += q.y; acc[c + 2] += q.z; acc[c + 3] += q.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] += f[c];
    }
  }
  const float denom = (float)cnt;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    if (c0 + c < p.C) volume[(int64_t)(c0 + c) * G + g] = cnt > 0 ? acc[c] / denom : 0.0f;
  }
  if (blockIdx.y == 0) count[g] = cnt;
}

// ---- pipelined cooperative-gather kernel (round 3; the product kernel) ------------------------------------------------
// The same arithmetic as backproject_accum_coop_kernel (results bit-identical; which lane gathers and stores for which voxel
// of the wave is group_src_lane()'s choice), but built for memory-level parallelism.  The round-2 loop put every gather
// inside its own conditional block, and the compiler closed each with `s_waitcnt vmcnt(0)`: ONE 1-KB gather in flight per wave, 24 KB per CU -- the kernel was bound
// by the latency of a single L2 / Infinity-Cache / HBM round trip (its run time scaled 1:1 with the number of resident
// waves), not by bandwidth.  Here all LPV gathers of a view are issued back to back (exec-masked loads,
// no branch in between), the projection of the NEXT view is computed while they fly, and only then are they added; with
// PIPE = 2 the gathers of view v + 1 are issued before the sums of view v.
//
// Schedule (SlabOrder + lockstep): the grid is cut into bricks; a brick is the unit one XCD group works on.  In lockstep
// mode the launch is a persistent grid of 8 x `bpc` workgroups (bpc = workgroups per brick, all resident): group g =
// blockIdx.x % 8 walks bricks g, g + 8, ... and meets at a group-local barrier after every brick, so that the workgroups
// sharing an L2 are in the same 32^3 box AND at about the same view at the same time -- the condition under which a
// pixel line fetched for one voxel is still in L2 when the next voxel on that camera ray asks for it
// (scripts/dense_l2sim.cpp: read hit rate 34 % -> 54 %, fabric reads 51 -> 35 GB per launch at the north-star shape).
// The barrier spins a bounded number of times: placement (b % 8 = XCD) and co-residency are performance assumptions,
// never correctness ones.
// Group-local barrier on ONE monotonic arrival counter (never reset, so a call that timed out leaves nothing to clean up):
// the k-th arrival waits until the counter reaches the next multiple of n.  Bounded spin: if the workgroups of a group
// are not all resident (another kernel holds CUs) the wait gives up after ~1 ms and the kernel merely loses its phase lock.
__device__ __forceinline__ void group_barrier(unsigned int* w, unsigned int n) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int old = __hip_atomic_fetch_add(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned int goal = (old / n + 1u) * n;
    for (int spin = 0; spin < 1024; ++spin) {             // sparse polls: every poll is an uncached memory transaction that
      if ((int)(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - goal) >= 0) break;     // competes with the
      __builtin_amdgcn_s_sleep(64);                        // gathers of the workgroups still at work (~1.7 us apart)
    }
  }
  __syncthreads();
}

// Which lane's voxel a lane accumulates as its group `grp` (lane = vsel * LPV + sub; the LPV lanes of one vsel read one pixel
// line together).  Any bijection works for the gathers: an instruction touches 64 / LPV pixel lines either way.
//   EPI == 0, LPV >= 4 (product): runs of 4 consecutive lanes -- lane (sub, vsel) owns voxels vsel*4 .. vsel*4+3 of every block of
//   4*VPG lanes, i.e. 4 consecutive z of one column, so its four accumulators of a channel are four consecutive floats of a
//   [C][X][Y][Z] plane and leave as ONE 16-byte store: a store instruction writes 16 * VPG contiguous bytes in each of LPV planes
//   (8 whole 128-byte lines at LPV = 8).
//   otherwise: voxel grp*VPG + vsel (a store instruction writes 4 * VPG bytes in each of LPV planes: 32-byte pieces at LPV = 8;
//   EPI == 2 keeps this form selectable for A/B runs in the experiments library).
template <int LPV, int EPI>
__device__ __forceinline__ int group_src_lane(int grp, int vsel) {
  constexpr int VPG = 64 / LPV;
  if constexpr (EPI == 0 && LPV >= 4) return (grp / 4) * (4 * VPG) + vsel * 4 + (grp % 4);
  else return grp * VPG + vsel;
}

typedef float dense_f4 __attribute__((ext_vector_type(4)));
typedef unsigned int dense_u4 __attribute__((ext_vector_type(4)));

// element type of the feature maps, what one 16-byte gather holds (vec_t: the same as a native vector, the type the gather is
// loaded as) and how many float4 accumulators (Q) it feeds
template <int ELEM> struct DenseElem { typedef float type; typedef float4 load_t; typedef dense_f4 vec_t; static constexpr int Q = 1; };
template <> struct DenseElem<CNRMA_ELEM_F16> { typedef uint16_t type; typedef uint4 load_t; typedef dense_u4 vec_t; static constexpr int Q = 2; };
template <> struct DenseElem<CNRMA_ELEM_BF16> { typedef uint16_t type; typedef uint4 load_t; typedef dense_u4 vec_t; static constexpr int Q = 2; };

// one 16-byte store of a z-run.  policy 0: plain, 1: non-temporal, 2: sc1 (write-through: the line is not kept in the XCD's L2)
__device__ __forceinline__ void store_run(float* o, float a, float b, float c, float d, int policy) {
  dense_f4 v = {a, b, c, d};
  if (policy == 1) __builtin_nontemporal_store(v, reinterpret_cast<dense_f4*>(o));
  else if (policy == 2) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(o), "v"(v) : "memory");
  else *reinterpret_cast<dense_f4*>(o) = v;
}

// EPI: 0 direct stores, z-run lane mapping (16-byte stores)   1 LDS-transposed stores   2 direct stores, round-3 lane mapping
// ELEM: 0 fp32 maps (a lane gathers 4 channels per 16-byte load), CNRMA_ELEM_F16 / CNRMA_ELEM_BF16 16-bit maps (8 channels per
// 16-byte load, widened exactly and summed in fp32: the same sums as on the widened maps); feat points at elements of that type
// the voxel of thread `tid` of logical block `lb`: is it in the grid, its world position and its linear index (-1 outside)
__device__ __forceinline__ bool block_voxel(const DenseParams& p, const SlabOrder& ord, int64_t lb, int tid, float* wx, float* wy,
                                            float* wz, int64_t* lin) {
  *wx = 0.f; *wy = 0.f; *wz = 0.f; *lin = -1;
  bool in_grid;
  if (ord.on) {
    int x = 0, y = 0, z = 0;
    in_grid = ord.on == 2 ? lattice_decode(p, ord, lb, tid, &x, &y, &z) : block_decode(p, ord, lb, tid, &x, &y, &z);
    if (in_grid) {
      *lin = ((int64_t)x * p.Y + y) * p.Z + z;
      *wx = (float)x * p.vs + p.ox; *wy = (float)y * p.vs + p.oy; *wz = (float)z * p.vs + p.oz;      // as voxel_world()
    }
  } else {
    const int64_t g = lb * 256 + tid;
    in_grid = g < (int64_t)p.X * p.Y * p.Z;
    if (in_grid) { voxel_world(p, g, wx, wy, wz); *lin = g; }
  }
  return in_grid;
}

// View masks.  At the north-star shape 68 % of the (wave, view) pairs are empty -- none of the wave's 64 voxels projects into the
// view --, and an empty view step still costs a whole projection (42 vector instructions), repeated identically in each of the 8
// channel sweeps.  The first sweep, launched on its own, therefore records what it finds out anyway: wave w of logical block lb
// writes one 64-bit word per 64 views at vmask[(lb * 4 + w) * ceil(V / 64)], bit v % 64 of word v / 64 set iff its ballot
// "any lane valid" was non-zero for view v.  The other sweeps -- a second launch on the same stream, same grid in x, same block
// remap, same voxel decode, same project() on the same lanes -- walk the set bits only.  Every word they read was written by the
// first launch (a wave outside the grid writes nothing and reads nothing), so the table needs no clearing.
// vmask: the table to walk (PIPE == 1 only), or NULL: every view is walked; vmask_out: the table to record into, or NULL
template <int LPV, int PIPE, int EPI, int ELEM = 0>
__device__ __forceinline__ void accum_block(const DenseParams& p, const typename DenseElem<ELEM>::type* __restrict__ feat,
                                            const float* __restrict__ proj, float* __restrict__ volume,
                                            int32_t* __restrict__ count, int64_t lb, int c0, bool write_count,
                                            const SlabOrder& ord, float* __restrict__ lds_wave, int tid,
                                            const unsigned long long* __restrict__ vmask = nullptr,
                                            unsigned long long* __restrict__ vmask_out = nullptr) {
  constexpr int VPG = 64 / LPV;
  constexpr int Q = DenseElem<ELEM>::Q, CPL = 4 * Q;        // float4 accumulators / channels per lane and voxel
  typedef typename DenseElem<ELEM>::type feat_t;
  typedef typename DenseElem<ELEM>::load_t load_t;
  typedef typename DenseElem<ELEM>::vec_t vec_t;
  static_assert(EPI != 1 || ELEM == 0, "the LDS-transposed epilogue exists for fp32 maps only");
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  const int lane = tid & 63;
  float wx, wy, wz;
  int64_t lin;
  bool in_grid = block_voxel(p, ord, lb, tid, &wx, &wy, &wz, &lin);
  if (__ballot(in_grid) == 0ull) return;
  float4 acc[LPV * Q];
#pragma unroll
  for (int i = 0; i < LPV * Q; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  int cnt = 0;
  int sub = lane % LPV, vsel = lane / LPV;
  const int64_t plane = (int64_t)p.H * p.W * p.C;
  const feat_t* fbase = feat + c0 + CPL * sub;

  auto pixel_of = [&](int v) -> int {
    float rx, ry;
    const bool ok = in_grid && project(proj + v * 12, wx, wy, wz, p.H, p.W, &rx, &ry);
    return ok ? ((int)ry * p.W + (int)rx) : -1;
  };
  auto gather = [&](int v, int pix, load_t* q) {
    // All LPV shuffles first, then LPV loads from the GLOBAL address space.  The maps' address may come out of memory (by
    // reference), so the compiler took the pointer for a generic one and gathered with flat loads, which count in lgkmcnt like
    // the shuffles: each load then sat behind a wait that also covered the flat loads before it.  Now the waits between
    // shuffles and loads count shuffles only and the loads are global_load_dwordx4 with nothing but vmcnt on them.
    const feat_t* fv = fbase + v * plane;
    int pq[LPV];
#pragma unroll
    for (int grp = 0; grp < LPV; ++grp) pq[grp] = __shfl(pix, group_src_lane<LPV, EPI>(grp, vsel), 64);
#pragma unroll
    for (int grp = 0; grp < LPV; ++grp) {
      if constexpr (ELEM == 0) q[grp] = make_float4(0.f, 0.f, 0.f, 0.f);
      else q[grp] = make_uint4(0u, 0u, 0u, 0u);             // +0.0 in either 16-bit type
      if (pq[grp] >= 0) {
        const vec_t t = *(const __attribute__((address_space(1))) vec_t*)(fv + (int64_t)pq[grp] * p.C);
        q[grp].x = t.x; q[grp].y = t.y; q[grp].z = t.z; q[grp].w = t.w;
      }
    }
  };
  auto add = [&](const load_t* q) {
#pragma unroll
    for (int grp = 0; grp < LPV; ++grp) {
      if constexpr (ELEM == 0) {
        acc[grp].x += q[grp].x; acc[grp].y += q[grp].y; acc[grp].z += q[grp].z; acc[grp].w += q[grp].w;
      } else {
        float4 a, b;
        elem16_x8<ELEM>(q[grp], &a, &b);
        acc[2 * grp].x += a.x; acc[2 * grp].y += a.y; acc[2 * grp].z += a.z; acc[2 * grp].w += a.w;
        acc[2 * grp + 1].x += b.x; acc[2 * grp + 1].y += b.y; acc[2 * grp + 1].z += b.z; acc[2 * grp + 1].w += b.w;
      }
    }
  };

  if constexpr (PIPE == 1) {
    // The views to walk, 64 per word: the wave's words of the first sweep's table (scalar loads: the address is wave-uniform), or
    // all views without a table.  A view whose bit is clear has no valid lane in this wave -- the bit is the ballot of the very
    // pixel_of() below on these lanes --, so skipping it changes no sum, no count and no order.  All of this is scalar work.
    const int nw = (p.V + 63) >> 6;
    const int64_t wave_words = (lb * 4 + __builtin_amdgcn_readfirstlane(tid >> 6)) * nw;
    const unsigned long long* wm = vmask != nullptr ? vmask + wave_words : nullptr;
    unsigned long long seen = 0ull;                        // recording: the views of the current word with a valid lane
    auto word = [&](int w) -> unsigned long long {
      if (wm != nullptr) return wm[w];
      const int left = p.V - 64 * w;
      return left >= 64 ? ~0ull : (1ull << left) - 1ull;
    };
    int w = 0;
    unsigned long long m = word(0);
    auto next_view = [&]() -> int {                        // the next set bit, -1 after the last
      while (m == 0ull) {
        if (++w >= nw) return -1;
        m = word(w);
      }
      const int v = 64 * w + __builtin_ctzll(m);
      m &= m - 1ull;
      return v;
    };
    int v = next_view();
    int pix_n = v >= 0 ? pixel_of(v) : -1;
    while (v >= 0) {
      const int pix = pix_n;
      const bool any = __ballot(pix >= 0) != 0ull;
      load_t q[LPV];
      if (any) gather(v, pix, q);
      cnt += pix >= 0 ? 1 : 0;
      const int vn = next_view();
      if (vmask_out != nullptr) {                          // recording walks every view, so every word is met and written
        if (any) seen |= 1ull << (v & 63);
        if (vn < 0 || (vn >> 6) != (v >> 6)) {
          if (lane == 0) vmask_out[wave_words + (v >> 6)] = seen;
          seen = 0ull;
        }
      }
      pix_n = vn >= 0 ? pixel_of(vn) : -1;                 // overlaps with the gathers in flight
      if (any) add(q);
      v = vn;
    }
  } else {
    // two views in flight: q0 holds view v (issued one iteration ago), q1 is issued for view v + 1 before q0 is consumed
    load_t q0[LPV], q1[LPV];
    int pix0 = pixel_of(0);
    bool any0 = __ballot(pix0 >= 0) != 0ull;
    if (any0) gather(0, pix0, q0);
    cnt += pix0 >= 0 ? 1 : 0;
    for (int v = 0; v < p.V; ++v) {
      bool any1 = false;
      if (v + 1 < p.V) {
        const int pix1 = pixel_of(v + 1);
        any1 = __ballot(pix1 >= 0) != 0ull;
        if (any1) gather(v + 1, pix1, q1);
        cnt += pix1 >= 0 ? 1 : 0;
      }
      if (any0) add(q0);
      any0 = any1;
#pragma unroll
      for (int grp = 0; grp < LPV; ++grp) q0[grp] = q1[grp];
    }
  }

  if constexpr (ELEM != 0 && LPV >= 8) {
    // 64 accumulators + 32 gather registers: what the epilogue needs (the voxel's linear index, the lane's place in its group) is
    // re-derived from a laundered thread index, so that none of it is live across the view loop
    int t2 = tid;
    asm volatile("" : "+v"(t2));
    sub = (t2 & 63) % LPV; vsel = (t2 & 63) / LPV;
    int x = 0, y = 0, z = 0;
    const int64_t g2 = lb * 256 + t2;
    bool in2;
    if (ord.on) in2 = ord.on == 2 ? lattice_decode(p, ord, lb, t2, &x, &y, &z) : block_decode(p, ord, lb, t2, &x, &y, &z);
    else { in2 = g2 < G; z = (int)(g2 % p.Z); y = (int)((g2 / p.Z) % p.Y); x = (int)(g2 / p.Z / p.Y); }
    in_grid = in2;
    lin = in2 ? ((int64_t)x * p.Y + y) * p.Z + z : -1;
  }
  // means.  The count and the linear index of the voxel a lane accumulates for (group grp) live in lane group_src_lane(grp).
  if constexpr (EPI == 0 && LPV >= 4) {
    // z-run mapping: groups 4r .. 4r+3 of a lane are 4 consecutive lanes' voxels.  A run leaves as one 16-byte store per channel
    // when its four voxels are in the grid at consecutive linear indices starting at a multiple of 4, with G % 4 == 0 and a
    // 16-byte aligned volume (then every plane's run is 16-byte aligned); otherwise (ragged bricks, Z % 4 != 0, odd grids,
    // offset output views) that run is stored element by element.  Decided per run; all shuffles are outside the branches.
    const bool vec_ok = (G & 3) == 0 && (reinterpret_cast<uintptr_t>(volume) & 15) == 0;
    const int c = c0 + CPL * sub;
#pragma unroll
    for (int r = 0; r < LPV / 4; ++r) {
      int64_t gv[4];
      float m[4][CPL];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int src = group_src_lane<LPV, EPI>(4 * r + k, vsel);
        const int cv = __shfl(cnt, src, 64);
        const int lo = __shfl((int)(lin & 0xffffffffLL), src, 64), hi = __shfl((int)(lin >> 32), src, 64);
        gv[k] = ((int64_t)hi << 32) | (uint32_t)lo;
        const float denom = (float)cv;
#pragma unroll
        for (int h = 0; h < Q; ++h) {
          const float4 a = acc[(4 * r + k) * Q + h];
          m[k][4 * h + 0] = cv > 0 ? a.x / denom : 0.0f; m[k][4 * h + 1] = cv > 0 ? a.y / denom : 0.0f;
          m[k][4 * h + 2] = cv > 0 ? a.z / denom : 0.0f; m[k][4 * h + 3] = cv > 0 ? a.w / denom : 0.0f;
        }
      }
      const bool whole = vec_ok && gv[0] >= 0 && (gv[0] & 3) == 0 && gv[1] == gv[0] + 1 && gv[2] == gv[0] + 2 && gv[3] == gv[0] + 3;
      if (whole) {
        float* o = volume + (int64_t)c * G + gv[0];
#pragma unroll
        for (int j = 0; j < CPL; ++j) store_run(o + j * G, m[0][j], m[1][j], m[2][j], m[3][j], ord.nt);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (gv[k] >= 0) {
            float* o = volume + (int64_t)c * G + gv[k];
#pragma unroll
            for (int j = 0; j < CPL; ++j) o[j * G] = m[k][j];
          }
      }
    }
  } else if constexpr (EPI != 1) {
#pragma unroll
    for (int grp = 0; grp < LPV; ++grp) {
      const int src = group_src_lane<LPV, EPI>(grp, vsel);
      const int cv = __shfl(cnt, src, 64);
      const int lo = __shfl((int)(lin & 0xffffffffLL), src, 64), hi = __shfl((int)(lin >> 32), src, 64);
      const int64_t gv = ((int64_t)hi << 32) | (uint32_t)lo;
      if (gv >= 0) {
        const float denom = (float)cv;
#pragma unroll
        for (int h = 0; h < Q; ++h) {
          const float4 a = acc[grp * Q + h];
          const int c = c0 + CPL * sub + 4 * h;
          const float m0 = cv > 0 ? a.x / denom : 0.0f, m1 = cv > 0 ? a.y / denom : 0.0f, m2 = cv > 0 ? a.z / denom : 0.0f,
                      m3 = cv > 0 ? a.w / denom : 0.0f;
          float* o = volume + (int64_t)c * G + gv;
          if (ord.nt == 1) {                      // streaming stores: the volume is written once and not read here
            __builtin_nontemporal_store(m0, o); __builtin_nontemporal_store(m1, o + G);
            __builtin_nontemporal_store(m2, o + 2 * G); __builtin_nontemporal_store(m3, o + 3 * G);
          } else { o[0] = m0; o[G] = m1; o[2 * G] = m2; o[3 * G] = m3; }
        }
      }
    }
  } else {
    // transpose through the wave's own LDS tile [4*LPV channels][64 voxels (+1 pad)] so that every store instruction
    // writes ONE channel plane for the wave's 64 voxels (two full 128-B lines in brick order) instead of 8 planes x 32 B
    constexpr int LD = 65;
    // everything the epilogue needs is re-derived here from a laundered thread index, so that nothing of it is live
    // across the view loop (kept live it pushed the loop over its 128 registers: scratch reloads = a vmcnt(0) per view)
    int t2 = tid;
    asm volatile("" : "+v"(t2));
    const int lane2 = t2 & 63, sub2 = lane2 % LPV, vsel2 = lane2 / LPV;
    float* ldsw = lds_wave + 0 * (t2 & 0);
#pragma unroll
    for (int grp = 0; grp < LPV; ++grp) {
      const int cv = __shfl(cnt, grp * VPG + vsel2, 64);
      const float denom = (float)cv;
      const float4 a = acc[grp];
      float* t = ldsw + (4 * sub2) * LD + grp * VPG + vsel2;
      t[0 * LD] = cv > 0 ? a.x / denom : 0.0f;
      t[1 * LD] = cv > 0 ? a.y / denom : 0.0f;
      t[2 * LD] = cv > 0 ? a.z / denom : 0.0f;
      t[3 * LD] = cv > 0 ? a.w / denom : 0.0f;
    }
    __builtin_amdgcn_wave_barrier();
    if (in_grid) {
      float* o = volume + (int64_t)c0 * G + lin;
#pragma unroll
      for (int c = 0; c < 4 * LPV; ++c) o[(int64_t)c * G] = ldsw[c * LD + lane2];
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (write_count && in_grid) count[lin] = cnt;
}

template <int LPV, int PIPE, int EPI, int LOCK>
__global__ __launch_bounds__(256, PIPE == 1 ? 4 : 3) void backproject_accum_pipe_kernel(DenseParams p, const float* feat,
                                                                     const float* __restrict__ proj,
                                                                     float* __restrict__ volume,
                                                                     int32_t* __restrict__ count, int chunk_blocks,
                                                                     int64_t n_phys, SlabOrder ord,
                                                                     unsigned int* __restrict__ bar,
                                                                     const float* const* __restrict__ feat_ref,
                                                                     const unsigned long long* __restrict__ vmask,
                                                                     unsigned long long* __restrict__ vmask_out, int sweep0) {
  // feat_ref != NULL: the feature maps are handed over BY REFERENCE -- a device word holds their address (one scalar load);
  // a captured launch sequence can then read whatever tensor the producer wrote, with no copy into a static buffer
  if (feat_ref != nullptr) feat = *feat_ref;
  __shared__ float lds[EPI == 1 ? 4 * (4 * LPV) * 65 : 1];
  float* lds_wave = lds + (EPI == 1 ? (threadIdx.x >> 6) * (4 * LPV) * 65 : 0);
  if constexpr (LOCK != 0) {
    // persistent grid: gridDim.x = 8 * chunk_blocks; group = blockIdx.x & 7 walks chunks group, group + 8, ...; all channel
    // sweeps inside (blockIdx.y unused)
    // ord.groups = 8: one brick per XCD at a time; 16: two independent groups per XCD (b and b + 8 share an XCD), each on its
    // own brick behind its own barrier -- while one group drains / decodes / projects, the other one's gathers keep the
    // memory pipeline busy
    const int NG = ord.groups;
    const int grp = blockIdx.x % NG, slot = blockIdx.x / NG;
    const int64_t n_chunks = n_phys / chunk_blocks;
    const int n_sweeps = (int)ceil_div_dev(p.C, 4 * LPV);
    for (int sw = 0; sw < n_sweeps; ++sw)
      for (int64_t ch = grp; ch < n_chunks; ch += NG) {
        // stagger: released together, the waves of a CU would project at the same time and then wait for memory at the
        // same time (lockstep 2x slower than free-running); wave w of every workgroup starts w x stagger x 64 cycles late,
        // so that at any moment a quarter of the waves is in each quarter of the view step
        for (int i = 0; i < ord.stagger * (int)(threadIdx.x >> 6); ++i) __builtin_amdgcn_s_sleep(1);
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));            // per-thread values are recomputed per brick instead of being hoisted out of
                                                 // the brick loop (hoisted they spilled, and a scratch access in the view loop
                                                 // puts a vmcnt(0) in front of every gather)
        accum_block<LPV, PIPE, EPI>(p, feat, proj, volume, count, ch * chunk_blocks + slot, sw * 4 * LPV, sw == 0, ord, lds_wave, tid);
        group_barrier(bar + grp * 16, (unsigned)chunk_blocks);
      }
  } else {
    int64_t lb = blockIdx.x;
    int sweep = blockIdx.y + sweep0;                     // sweep0: first channel sweep of this launch
    if (ord.own > 0) {
      // one channel sweep per XCD group (8 sweeps <-> 8 groups): every group walks ALL bricks in order for its own 128-byte
      // slice of the pixel rows, so the workgroups resident on an XCD are one contiguous run of neighbouring bricks (not
      // every 8th brick) and no feature line is fetched by two XCDs (dense_l2sim: read hit rate 34 % -> 41 %)
      sweep = (int)(lb & 7);
      lb >>= 3;
    } else lb = remap_block(blockIdx.x, chunk_blocks, ord);
    accum_block<LPV, PIPE, EPI>(p, feat, proj, volume, count, lb, sweep * (4 * LPV), sweep == 0, ord, lds_wave, (int)threadIdx.x, vmask, vmask_out);
  }
}

// The product schedule of the kernel above (one view in flight, z-run stores, free-running brick order) on 16-bit maps: a lane
// gathers 8 channels per 16-byte load, so LPV lanes cover 8 * LPV channels per sweep.  OCC = waves per SIMD the register
// budget is cut for (3 only for the 8-lane form, whose 64 accumulators + 32 gather registers do not fit 128).
template <int LPV, int ELEM, int OCC>
__global__ __launch_bounds__(256, OCC) void backproject_accum_h16_kernel(DenseParams p, const uint16_t* feat,
                                                                         const float* __restrict__ proj,
                                                                         float* __restrict__ volume,
                                                                         int32_t* __restrict__ count, int chunk_blocks,
                                                                         SlabOrder ord,
                                                                         const uint16_t* const* __restrict__ feat_ref,
                                                                         const unsigned long long* __restrict__ vmask,
                                                                         unsigned long long* __restrict__ vmask_out, int sweep0) {
  if (feat_ref != nullptr) feat = *feat_ref;               // by reference, as backproject_accum_pipe_kernel
  const int64_t lb = remap_block(blockIdx.x, chunk_blocks, ord);
  const int sweep = blockIdx.y + sweep0;
  accum_block<LPV, 1, 0, ELEM>(p, feat, proj, volume, count, lb, sweep * (8 * LPV), sweep == 0, ord, nullptr, (int)threadIdx.x, vmask, vmask_out);
}

#ifdef CNRMA_EXPERIMENTS
#include "dense_exp.inc"
#endif

// Debug / A-B switches of the dense kernel.  Product code never reads the environment: the defaults below ARE the shipped
// configuration, and only cnrma_debug_dense_tuning() (scripts/dense_ab.py, tests of the alternative orders) changes them.
struct DenseTune {
  int variant = 1;      // 0: round-2 kernel (one gather in flight per wave)   1: pipelined kernel   2: hoisted kernel
  int slab = 1;         // 1: brick order, 0: z-fastest linear order with x-plane chunks
  int st = 16, zt = 32, tt = 8, zi = 32;   // brick side (columns), brick layers, tile side, inner z run
  int chunk = -1;       // blocks per XCD chunk in linear order (-1: one x-plane, 0: plain round-robin)
  int persist = 0;      // variant 0 only: workgroups per CU of its persistent form
  int lpv = 0;          // 0: by channel count; 4 / 8 / 16 / 32 lanes (x 4 channels) per voxel
  int pipe = 1;         // variant 1: views in flight (1 | 2)
  int epi = 0;          // variant 1: 0 direct stores, 1 LDS-transposed full-line stores
  int nt = 0;           // variant 1: cache policy of the volume stores: 0 plain, 1 non-temporal, 2 sc1 (write-through; 16-byte stores only)
  int own = 0;          // variant 1: one channel sweep per XCD group (needs exactly 8 sweeps)
  int stagger = 0;      // variant 1 lockstep: start delay per wave index, in units of 64 cycles
  int ldspad = 0;       // variant 1: KB of unused dynamic LDS per workgroup (caps the workgroups per CU: leaves room for co-resident kernels)
  int groups = 8;       // variant 1 lockstep: 8 = one brick per XCD at a time, 16 = two independent half-size groups per XCD
  int lattice = 0;      // variant 1 lockstep: 1 = lattice assignment of columns to workgroups (balanced), 0 = compact tiles
  int lockstep = 0;     // variants 1, 2: persistent grid, every XCD group walks one brick at a time (1: behind a barrier, 2: no barrier)
  int zrun = 1;         // variant 1, epi 0: 1 = a lane owns runs of 4 consecutive z (16-byte stores), 0 = the round-3 lane mapping (4-byte stores)
};
#ifdef CNRMA_EXPERIMENTS
static DenseTune g_tune;                     // libcnrma_hip_exp.so only: written by cnrma_debug_dense_tuning
#define CNRMA_DENSE_TUNE g_tune
#else
// the product library has no tuning state: the defaults above ARE the shipped configuration (pipelined kernel, brick order)
static constexpr DenseTune k_dense_tune{};
#define CNRMA_DENSE_TUNE k_dense_tune
#endif

// the shift fields of a brick order whose sizes are powers of two, for a grid of gx blocks in chunks of cb blocks (remap_block()
// shifts by lcb, so the chunk must be exactly one brick)
static void slab_shifts(SlabOrder& o, int64_t gx, int64_t cb) {
  auto lg = [](int v) { int l = 0; while (l < 30 && (1 << l) < v) ++l; return (1 << l) == v ? l : -1; };
  const int lst = lg(o.st), lzt = lg(o.zt), ltt = lg(o.tt), lzi = lg(o.zi);
  if (lst < 0 || lzt < 0 || ltt < 0 || lzi < 0 || 2 * lst + lzt < 8 || gx >= ((int64_t)1 << 31) ||
      cb != ((int64_t)1 << (2 * lst + lzt - 8))) return;
  o.p2 = 1; o.lcb = 2 * lst + lzt - 8; o.lzi = lzi; o.ltt = ltt; o.lzo = lzt - lzi; o.ltpr = lst - ltt;
}

// The caller's workspace behind its first CNRMA_DENSE_WORKSPACE_BYTES as the view-mask table of a grid of gx blocks, or NULL (then
// one launch walks every view in every sweep, as it did before the table existed): the workspace must hold CNRMA_DENSE_MASK_BYTES behind the
// counters, and the table of this grid -- one word per wave and 64 views -- must fit into that.
static unsigned long long* view_mask_table(const DenseParams& p, void* workspace, int64_t workspace_bytes, int64_t gx) {
  const int64_t room = CNRMA_DENSE_MASK_BYTES(p.X, p.Y, p.Z, p.V);
  if (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || workspace_bytes < CNRMA_DENSE_WORKSPACE_BYTES + room) return nullptr;
  if (gx * 4 * ((p.V + 63) / 64) * 8 > room) return nullptr;
  return reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + CNRMA_DENSE_WORKSPACE_BYTES);
}

template <int LPV>
int launch_accum_coop(const DenseParams& p, const float* feat, const float* proj, float* volume, int32_t* count,
                      void* workspace, int64_t workspace_bytes, hipStream_t st, const float* const* feat_ref = nullptr) {
  unsigned int* bar = (workspace != nullptr && workspace_bytes >= CNRMA_DENSE_WORKSPACE_BYTES) ? static_cast<unsigned int*>(workspace) : nullptr;
  const DenseTune t = CNRMA_DENSE_TUNE;
  if (feat_ref != nullptr && t.variant != 1) return CNRMA_EINVAL;      // by-reference hand-off: the product kernel only
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  int64_t nb = ceil_div(G, 256);
  // one chunk = the blocks of one x-plane (at least 32: keeps a group's L2 working set a compact slab piece)
  int64_t cb = ceil_div((int64_t)p.Y * p.Z, 256);
  if (cb < 32) cb = 32;
  SlabOrder ord{0, 0, 0, 0, t.zt, t.st, t.tt, t.zi, t.nt, 0, t.stagger, t.groups == 16 ? 16 : 8};
  if (t.slab) {
    ord.on = 1;
    if (ord.zi < 1 || ord.zt % ord.zi != 0) return CNRMA_EINVAL;
    if (ord.zt < 1 || ord.tt < 1 || ord.st < ord.tt || ord.st % ord.tt != 0 || ((int64_t)ord.st * ord.st * ord.zt) % 256 != 0) return CNRMA_EINVAL;
    ord.nsx = (int)ceil_div(p.X, ord.st); ord.nsy = (int)ceil_div(p.Y, ord.st); ord.nsz = (int)ceil_div(p.Z, ord.zt);
    cb = (int64_t)ord.st * ord.st * ord.zt / 256;          // one brick per chunk
    nb = (int64_t)ord.nsx * ord.nsy * ord.nsz * cb;
  } else if (t.chunk >= 0) cb = t.chunk;
  int64_t gx = nb;
  if (cb > 0 && (nb >= 16 * cb || ord.on)) gx = ceil_div(ceil_div(nb, cb), 8) * 8 * cb;      // whole chunks for every XCD group
  else cb = 0;
  if (ord.on) slab_shifts(ord, gx, cb);
#ifdef CNRMA_EXPERIMENTS
  if (t.variant == 0) {
    int64_t launch_x = gx;
    if (t.persist > 0 && gx > (int64_t)256 * t.persist) launch_x = (int64_t)256 * t.persist;     // a multiple of 8
    dim3 grid((unsigned)launch_x, (unsigned)ceil_div(p.C, 4 * LPV));
    hipLaunchKernelGGL((backproject_accum_coop_kernel<LPV>), grid, dim3(256), 0, st, p, feat, proj, volume, count, (int)cb, gx, ord);
    CNRMA_LAUNCH_CHECK();
    return 0;
  }
  if (t.variant == 2 && p.V <= 64 && (int64_t)p.H * p.W * p.C * 4 < ((int64_t)1 << 31)) {
    const int lock = (t.lockstep && (bar != nullptr || t.lockstep == 2) && ord.on && ord.zt == 32 && ord.st % 8 == 0 && cb > 0 && cb <= 256) ? 1 : 0;
    const size_t lds = (size_t)4 * p.V * 64 * sizeof(int32_t);
    dim3 grid(lock ? (unsigned)(8 * cb) : (unsigned)gx);
    if (lock)
      hipLaunchKernelGGL((backproject_accum_hoist_kernel<LPV, 1>), grid, dim3(256), lds, st, p, feat, proj, volume, count, (int)cb,
                         gx, ord, bar, t.lockstep == 1 ? 1 : 0);
    else
      hipLaunchKernelGGL((backproject_accum_hoist_kernel<LPV, 0>), grid, dim3(256), lds, st, p, feat, proj, volume, count, (int)cb,
                         gx, ord, bar, 0);
    CNRMA_LAUNCH_CHECK();
    return 0;
  }
#endif
  const int lock = (t.lockstep == 1 && bar != nullptr && ord.on && cb > 0 && cb <= 256) ? 1 : 0;
  if (t.lattice && ord.on && ord.zt == 32 && ord.st % 8 == 0) ord.on = 2;
  const int n_sweeps = (int)ceil_div(p.C, 4 * LPV);
  if (t.own && !lock && ord.on && n_sweeps == 8 && nb * 8 < ((int64_t)1 << 31)) ord.own = 1;
  dim3 grid(lock ? (unsigned)(ord.groups * cb) : (ord.own ? (unsigned)(nb * 8) : (unsigned)gx), (lock || ord.own) ? 1u : (unsigned)n_sweeps);
  // the free-running grid with one view in flight and more than one sweep: the first sweep records the view masks, the others walk
  // them -- when the caller's workspace has room for the table
  unsigned long long* vmask = (!lock && !ord.own && t.pipe != 2 && n_sweeps > 1) ? view_mask_table(p, workspace, workspace_bytes, gx) : nullptr;
  auto launch = [&](dim3 grid, int sweep0, const unsigned long long* vin, unsigned long long* vout) -> int {
#ifdef CNRMA_EXPERIMENTS
#define CNRMA_DENSE_LAUNCH(PIPE, EPI)                                                                                      \
  do {                                                                                                                     \
    if (lock)                                                                                                              \
      hipLaunchKernelGGL((backproject_accum_pipe_kernel<LPV, PIPE, EPI, 1>), grid, dim3(256), 0, st, p, feat, proj, volume, \
                         count, (int)cb, gx, ord, bar, feat_ref, vin, vout, sweep0);                                       \
    else                                                                                                                   \
      hipLaunchKernelGGL((backproject_accum_pipe_kernel<LPV, PIPE, EPI, 0>), grid, dim3(256), (size_t)t.ldspad * 1024, st, p,  \
                         feat, proj, volume, count, (int)cb, gx, ord, bar, feat_ref, vin, vout, sweep0);                  \
  } while (0)
  if (t.pipe == 2) { if (t.epi) CNRMA_DENSE_LAUNCH(2, 1); else if (t.zrun) CNRMA_DENSE_LAUNCH(2, 0); else CNRMA_DENSE_LAUNCH(2, 2); }
  else             { if (t.epi) CNRMA_DENSE_LAUNCH(1, 1); else if (t.zrun) CNRMA_DENSE_LAUNCH(1, 0); else CNRMA_DENSE_LAUNCH(1, 2); }
#undef CNRMA_DENSE_LAUNCH
#else                                   // the product schedule: one view in flight per wave, direct 16-byte stores of z-runs, free-running grid
  hipLaunchKernelGGL((backproject_accum_pipe_kernel<LPV, 1, 0, 0>), grid, dim3(256), 0, st, p, feat, proj, volume, count, (int)cb, gx,
                     ord, bar, feat_ref, vin, vout, sweep0);
#endif
    CNRMA_LAUNCH_CHECK();
    return 0;
  };
  if (vmask == nullptr) return launch(grid, 0, nullptr, nullptr);
  const int rc = launch(dim3(grid.x, 1u), 0, nullptr, vmask);
  return rc != 0 ? rc : launch(dim3(grid.x, (unsigned)(n_sweeps - 1)), 1, vmask, nullptr);
}

__global__ __launch_bounds__(256) void backproject_index_kernel(DenseParams p, const float* __restrict__ proj,
                                                                int32_t* __restrict__ px, int32_t* __restrict__ py,
                                                                uint8_t* __restrict__ valid) {
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  float wx, wy, wz, rx, ry;
  voxel_world(p, g, &wx, &wy, &wz);
  bool ok = project(proj, wx, wy, wz, p.H, p.W, &rx, &ry);
  const float lim = 2147483000.0f;
  px[g] = (rx > -lim && rx < lim) ? (int32_t)rx : INT32_MIN;
  py[g] = (ry > -lim && ry < lim) ? (int32_t)ry : INT32_MIN;
  valid[g] = ok ? 1 : 0;
}

template <int CT>
int launch_accum(const DenseParams& p, const float* feat, const float* proj, float* volume, int32_t* count,
                 hipStream_t st) {
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  dim3 grid((unsigned)ceil_div(G, 256), (unsigned)ceil_div(p.C, CT));
  hipLaunchKernelGGL((backproject_accum_kernel<CT>), grid, dim3(256), 0, st, p, feat, proj, volume, count);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

}  // namespace

#ifdef CNRMA_EXPERIMENTS
extern "C" int cnrma_debug_dense_tuning(const int* v, int n) {
  // v = {variant, slab, st, zt, tt, zi, chunk, persist, lpv, pipe, epi, lockstep, lattice, nt, own, stagger, groups, ldspad, zrun}; n < 19 keeps the remaining defaults;
  // n == 0 restores the product configuration.  Host-side global state: debug / A-B runs only.
  DenseTune t;
  int* f[] = {&t.variant, &t.slab, &t.st, &t.zt, &t.tt, &t.zi, &t.chunk, &t.persist, &t.lpv, &t.pipe, &t.epi, &t.lockstep, &t.lattice, &t.nt, &t.own, &t.stagger, &t.groups, &t.ldspad, &t.zrun};
  if (n < 0 || n > 19 || (n > 0 && v == nullptr)) return CNRMA_EINVAL;
  for (int i = 0; i < n; ++i) *f[i] = v[i];
  g_tune = t;
  return 0;
}
#endif

static int backproject_accum_any(const float* feat_nhwc, const float* const* feat_ref, const float* proj, int V, int C, int H,
                                 int W, int X, int Y, int Z, float voxel_size, float ox, float oy, float oz, float* volume,
                                 int32_t* count, void* workspace, int64_t workspace_bytes, void* stream) {
  if (V <= 0 || C <= 0 || H <= 0 || W <= 0 || X <= 0 || Y <= 0 || Z <= 0) return CNRMA_EINVAL;
  DenseParams p{V, C, H, W, X, Y, Z, voxel_size, ox, oy, oz};
  hipStream_t st = as_stream(stream);
#ifdef CNRMA_EXPERIMENTS                // lanes per voxel by hand: the 16-lane form exists in the experiments library only
  const int l = CNRMA_DENSE_TUNE.lpv;
  if (l == 16 && C % 64 == 0) return launch_accum_coop<16>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
  if (l == 4 && C % 16 == 0) return launch_accum_coop<4>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
#endif
  if (C % 32 == 0) return launch_accum_coop<8>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
  if (C % 16 == 0) return launch_accum_coop<4>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
  if (C % 8 == 0) return launch_accum_coop<2>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
  if (C % 4 == 0) return launch_accum_coop<1>(p, feat_nhwc, proj, volume, count, workspace, workspace_bytes, st, feat_ref);
  if (feat_ref != nullptr) return CNRMA_EINVAL;
  return launch_accum<1>(p, feat_nhwc, proj, volume, count, st);
}

extern "C" int cnrma_backproject_accum_f32(const float* feat_nhwc, const float* proj, int V, int C, int H, int W,
                                           int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                           float* volume, int32_t* count, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  if (feat_nhwc == nullptr) return CNRMA_EINVAL;
  return backproject_accum_any(feat_nhwc, nullptr, proj, V, C, H, W, X, Y, Z, voxel_size, ox, oy, oz, volume, count, workspace,
                               workspace_bytes, stream);
}

extern "C" int cnrma_backproject_accum_ref_f32(const float* const* feat_nhwc_ref, const float* proj, int V, int C, int H, int W,
                                               int X, int Y, int Z, float voxel_size, float ox, float oy, float oz,
                                               float* volume, int32_t* count, void* workspace, int64_t workspace_bytes,
                                               void* stream) {
  if (feat_nhwc_ref == nullptr || C % 4 != 0) return CNRMA_EINVAL;
  return backproject_accum_any(nullptr, feat_nhwc_ref, proj, V, C, H, W, X, Y, Z, voxel_size, ox, oy, oz, volume, count,
                               workspace, workspace_bytes, stream);
}

// 16-bit maps: always the shipped schedule (DenseTune's defaults: brick order, one brick per XCD chunk); the A/B switches of the
// experiments library only choose between the two C % 64 == 0 forms (lpv = 4 | 8)
// lanes per voxel of the shipped C % 64 == 0 form: 8 = a whole 128-byte line per pixel and sweep at 3 waves per SIMD (168 VGPRs),
// 4 = a 64-byte half line at 4 waves per SIMD (100 VGPRs); both free of scratch.  Measured at the north-star shape (DESIGN.md,
// "Dense unprojection on 16-bit maps"; profiles/r08_dense_half_ab_ns.log): 4 lanes 10.47 / 10.42 ms (fp16 / bf16), 8 lanes
// 10.63 / 10.61 ms -- the 4-lane form ships
#define CNRMA_H16_LANES_C64 4

template <int LPV, int OCC>
static int launch_accum_h16(const DenseParams& p, const uint16_t* feat, const uint16_t* const* feat_ref, int elem, const float* proj,
                            float* volume, int32_t* count, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  constexpr DenseTune t{};
  SlabOrder ord{1, (int)ceil_div(p.X, t.st), (int)ceil_div(p.Y, t.st), (int)ceil_div(p.Z, t.zt), t.zt, t.st, t.tt, t.zi, t.nt, 0, 0, 8};
  const int64_t cb = (int64_t)t.st * t.st * t.zt / 256;                  // one brick per chunk
  const int64_t nb = (int64_t)ord.nsx * ord.nsy * ord.nsz * cb;
  const int64_t gx = ceil_div(ceil_div(nb, cb), 8) * 8 * cb;             // whole chunks for every XCD group
  slab_shifts(ord, gx, cb);
  const int n_sweeps = (int)ceil_div(p.C, 8 * LPV);
  unsigned long long* vmask = n_sweeps > 1 ? view_mask_table(p, workspace, workspace_bytes, gx) : nullptr;      // as launch_accum_coop
  auto launch = [&](dim3 grid, int sweep0, const unsigned long long* vin, unsigned long long* vout) -> int {
    if (elem == CNRMA_ELEM_F16)
      hipLaunchKernelGGL((backproject_accum_h16_kernel<LPV, CNRMA_ELEM_F16, OCC>), grid, dim3(256), 0, st, p, feat, proj, volume, count,
                         (int)cb, ord, feat_ref, vin, vout, sweep0);
    else
      hipLaunchKernelGGL((backproject_accum_h16_kernel<LPV, CNRMA_ELEM_BF16, OCC>), grid, dim3(256), 0, st, p, feat, proj, volume, count,
                         (int)cb, ord, feat_ref, vin, vout, sweep0);
    CNRMA_LAUNCH_CHECK();
    return 0;
  };
  if (vmask == nullptr) return launch(dim3((unsigned)gx, (unsigned)n_sweeps), 0, nullptr, nullptr);
  const int rc = launch(dim3((unsigned)gx, 1u), 0, nullptr, vmask);
  return rc != 0 ? rc : launch(dim3((unsigned)gx, (unsigned)(n_sweeps - 1)), 1, vmask, nullptr);
}

extern "C" int cnrma_backproject_accum_h16(const void* feat_nhwc, const void* const* feat_nhwc_ref, int elem, const float* proj,
                                           int V, int C, int H, int W, int X, int Y, int Z, float voxel_size, float ox, float oy,
                                           float oz, float* volume, int32_t* count, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  if (!elem16_known(elem) || (feat_nhwc == nullptr) == (feat_nhwc_ref == nullptr) || (reinterpret_cast<uintptr_t>(feat_nhwc) & 15) != 0)
    return CNRMA_EINVAL;
  if (V <= 0 || C <= 0 || C % 8 != 0 || H <= 0 || W <= 0 || X <= 0 || Y <= 0 || Z <= 0) return CNRMA_EINVAL;
  DenseParams p{V, C, H, W, X, Y, Z, voxel_size, ox, oy, oz};
  hipStream_t st = as_stream(stream);
  const uint16_t* f = static_cast<const uint16_t*>(feat_nhwc);
  const uint16_t* const* fr = reinterpret_cast<const uint16_t* const*>(feat_nhwc_ref);
#if defined(CNRMA_EXPERIMENTS) || CNRMA_H16_LANES_C64 == 8
  int lanes64 = CNRMA_H16_LANES_C64;
#ifdef CNRMA_EXPERIMENTS                // either C % 64 == 0 form by hand, for A/B runs (scripts/dense_half_ab.py)
  if (CNRMA_DENSE_TUNE.lpv == 8 || CNRMA_DENSE_TUNE.lpv == 4) lanes64 = CNRMA_DENSE_TUNE.lpv;
#endif
  if (C % 64 == 0 && lanes64 == 8) return launch_accum_h16<8, 3>(p, f, fr, elem, proj, volume, count, workspace, workspace_bytes, st);
#endif
  if (C % 32 == 0) return launch_accum_h16<4, 4>(p, f, fr, elem, proj, volume, count, workspace, workspace_bytes, st);
  if (C % 16 == 0) return launch_accum_h16<2, 4>(p, f, fr, elem, proj, volume, count, workspace, workspace_bytes, st);
  return launch_accum_h16<1, 4>(p, f, fr, elem, proj, volume, count, workspace, workspace_bytes, st);
}

// Backward of the accumulate + mean w.r.t. the feature maps (training): volume[c][g] = sum_v feat[v][pix_v(g)][c] / count[g],
// so every valid (voxel, view) pair adds grad_volume[c][g] / count[g] to grad_feat[v][pix][c].  ~58 voxels share a pixel:
// float atomics (sum order not fixed: training only).  One lane per (voxel, 4 channels): a wave adds 128-byte channel
// vectors, the shape the memory-side atomic units run at full rate for.
template <int LPV>
__global__ __launch_bounds__(256) void backproject_backward_kernel(DenseParams p, const float* __restrict__ grad_volume,
                                                                   const int32_t* __restrict__ count,
                                                                   const float* __restrict__ proj,
                                                                   float* __restrict__ grad_feat) {
  const int64_t G = (int64_t)p.X * p.Y * p.Z;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t g = t / LPV;
  const int sub = (int)(t % LPV);
  if (g >= G) return;
  const int cnt = count[g];
  if (cnt <= 0) return;
  float wx, wy, wz;
  voxel_world(p, g, &wx, &wy, &wz);
  const float denom = (float)cnt;
  const int64_t plane = (int64_t)p.H * p.W * p.C;
  for (int c = 4 * sub; c < p.C; c += 4 * LPV) {
    float gq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gq[j] = (c + j < p.C) ? grad_volume[(int64_t)(c + j) * G + g] / denom : 0.0f;
    for (int v = 0; v < p.V; ++v) {
      float rx, ry;
      if (!project(proj + v * 12, wx, wy, wz, p.H, p.W, &rx, &ry)) continue;
      float* q = grad_feat + v * plane + ((int64_t)(int)ry * p.W + (int)rx) * p.C + c;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < p.C) atomicAdd(q + j, gq[j]);
    }
  }
}

extern "C" int cnrma_backproject_backward_f32(const float* grad_volume, const int32_t* count, const float* proj, int V,
                                              int C, int H, int W, int X, int Y, int Z, float voxel_size, float ox,
                                              float oy, float oz, float* grad_feat_nhwc, void* stream) {
  if (V <= 0 || C <= 0 || H <= 0 || W <= 0 || X <= 0 || Y <= 0 || Z <= 0 || grad_volume == nullptr || count == nullptr ||
      grad_feat_nhwc == nullptr)
    return CNRMA_EINVAL;
  DenseParams p{V, C, H, W, X, Y, Z, voxel_size, ox, oy, oz};
  hipStream_t st = as_stream(stream);
  hipError_t e = cnrma_fill_bytes(grad_feat_nhwc, 0, (size_t)V * H * W * C * sizeof(float), st);
  if (e != hipSuccess) return -(int)e;
  const int64_t G = (int64_t)X * Y * Z;
  if (C >= 32) {
    hipLaunchKernelGGL((backproject_backward_kernel<8>), dim3((unsigned)ceil_div(G * 8, 256)), dim3(256), 0, st, p,
                       grad_volume, count, proj, grad_feat_nhwc);
  } else {
    hipLaunchKernelGGL((backproject_backward_kernel<1>), dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, st, p, grad_volume,
                       count, proj, grad_feat_nhwc);
  }
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_backproject_index_f32(const float* proj_view, int H, int W, int X, int Y, int Z, float voxel_size,
                                           float ox, float oy, float oz, int32_t* px, int32_t* py, uint8_t* valid,
                                           void* stream) {
  if (H <= 0 || W <= 0 || X <= 0 || Y <= 0 || Z <= 0) return CNRMA_EINVAL;
  DenseParams p{1, 1, H, W, X, Y, Z, voxel_size, ox, oy, oz};
  const int64_t G = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(backproject_index_kernel, dim3((unsigned)ceil_div(G, 256)), dim3(256), 0, as_stream(stream), p,
                     proj_view, px, py, valid);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
