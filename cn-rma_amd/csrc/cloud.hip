// Point clouds on the device: voxel down-sample, exact nearest neighbour and the sums behind the mesh metrics (reference:
// post_process/evaluate_mesh.py:29-92, which calls Open3D's voxel_down_sample and a KDTreeFlann queried vertex by vertex).
// Points are [N][3] fp32, row-major; every data-dependent row count is a device word; include/cnrma.h (a15) holds the contracts.
//
// down-sample:  fp32 minimum per axis (exact) -> fp64 voxel keys packed 3 x 21 bits -> stable radix sort of (key, index) ->
//               segment heads -> scan -> one thread per voxel sums its points in fp64 in ascending input index
// nn build:     bounding box -> one thread derives the cell size and the dims (<= 2^24 cells) into a device header -> cell ids
//               (z fastest) + histogram -> scan of the live cells -> radix sort of (cell, index) -> 16-byte records {x, y, z, index}
// nn query:     one query per lane; Chebyshev shells around the query's (clamped) cell, one contiguous record range per (x, y)
//               row of a shell; the running best is the pair (d2, index); stop once the best is strictly inside the distance to
//               every face of the visited block that is not the grid's boundary (less a margin for the cell assignment's rounding)
// The nearest neighbour is a function of the two clouds alone (fp64, un-fused, ties to the lowest index): not of the grid, the
// cell size or the visiting order.  No tuning state, nothing read from the environment, no allocation, no synchronisation.
#include <math.h>

#include "common.h"

#include <hipcub/hipcub.hpp>

namespace {

constexpr int CLOUD_BLOCK = 256;
constexpr int64_t CLOUD_MAX_POINTS = ((int64_t)1 << 31) - 2;      // every row number, and n + 1 scan entries, stay inside int32
constexpr int CLOUD_KEY_BITS = 21;
constexpr int64_t CLOUD_MAX_CELLS = (int64_t)1 << 24;
constexpr int CLOUD_SCAN_BLOCKS = 1024;                           // chunks of the cell scan
constexpr int CLOUD_SCAN_TILE = CLOUD_BLOCK * 4;

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

template <typename K>
size_t cloud_sort_temp_bytes(int64_t n) {
  size_t bytes = 0;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const K*)nullptr, (K*)nullptr, (const int32_t*)nullptr,
                                                    (int32_t*)nullptr, (int)n, 0, (int)sizeof(K) * 8, nullptr);
  if (e != hipSuccess || bytes == 0) bytes = (size_t)n * 16 + (1u << 20);      // no device: an estimate, as in sparse.hip
  (void)hipGetLastError();
  return align256(bytes);
}

// order-preserving map fp32 -> uint32, so that a minimum / maximum over floats is an integer atomic
__device__ __forceinline__ uint32_t f32_ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_ordered(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ bool f32_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// lo[3] / hi[3] (ordered words) and a flags word.  Non-finite rows set CNRMA_CLOUD_NONFINITE and do not count.
struct CloudBox { uint32_t lo[3], hi[3]; int32_t flags, pad; };

__global__ void cloud_box_init_kernel(CloudBox* box) {
  for (int a = 0; a < 3; ++a) { box->lo[a] = 0xffffffffu; box->hi[a] = 0u; }
  box->flags = 0;
  box->pad = 0;
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_box_kernel(const float* __restrict__ pts, int64_t n_cap,
                                                                const int32_t* __restrict__ n_dev, CloudBox* box) {
  const int64_t n = live_rows(n_cap, n_dev);
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * CLOUD_BLOCK) {
    const float x = pts[i * 3], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
    if (!(f32_finite(x) && f32_finite(y) && f32_finite(z))) { bad = true; continue; }
    const uint32_t o[3] = {f32_ordered(x), f32_ordered(y), f32_ordered(z)};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], o[a]); hi[a] = max(hi[a], o[a]); }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = wave_min_u32(lo[a]); hi[a] = wave_max_u32(hi[a]); }
  // one set of atomics per block, from few blocks: six words that every block hits serialise in L2 (a set per wave from a grid
  // over all points took 190 us for 2 x 10^5 points)
  __shared__ uint32_t s_box[CLOUD_BLOCK / 64][6];
  const int any_bad = __syncthreads_or((int)bad);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { s_box[threadIdx.x >> 6][a] = lo[a]; s_box[threadIdx.x >> 6][3 + a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    uint32_t v = s_box[0][a];
    for (int w = 1; w < CLOUD_BLOCK / 64; ++w) v = a < 3 ? min(v, s_box[w][a]) : max(v, s_box[w][a]);
    if (a < 3) { if (v != 0xffffffffu) atomicMin(&box->lo[a], v); }
    else if (v != 0u) atomicMax(&box->hi[a - 3], v);
  }
  if (threadIdx.x == 0 && any_bad) atomicOr(&box->flags, CNRMA_CLOUD_NONFINITE);
}

unsigned cloud_grid(int64_t n, int64_t most = 4096) {
  int64_t b = ceil_div(n, CLOUD_BLOCK);
  return (unsigned)(b < 1 ? 1 : (b > most ? most : b));
}
constexpr int64_t CLOUD_BOX_BLOCKS = 128;

// ================================================================================================================
// voxel down-sample
// ================================================================================================================
struct DownLayout {
  size_t box, key_a, key_b, val_a, val_b, head, off, sort_tmp, sort_tmp_bytes, scan, total;
};

DownLayout down_layout(int64_t n) {
  DownLayout L{};
  const size_t n4 = (size_t)((n + 3) / 4 * 4);
  size_t p = 0;
  L.box = p; p += 256;
  L.key_a = p; p += align256(n4 * 8);
  L.key_b = p; p += align256(n4 * 8);
  L.val_a = p; p += align256(n4 * 4);
  L.val_b = p; p += align256(n4 * 4);
  L.head = p; p += align256(n4 * 4);
  L.off = p; p += align256((n4 + 4) * 4);
  L.sort_tmp_bytes = cloud_sort_temp_bytes<uint64_t>(n > 0 ? n : 1);
  L.sort_tmp = p; p += L.sort_tmp_bytes;
  L.scan = p; p += align256(cnrma_scan_workspace_bytes(n > 0 ? n : 1));
  L.total = p;
  return L;
}

// key of row i: k[a] = floor(((double)p[a] - org[a]) / vs), org[a] = (double)lo[a] - 0.5 vs; 21 bits per axis, x on top.
// Dead rows, and every row once a flag is up, carry the all-ones key: they sort behind the live rows (the sort is stable and their
// indices are the highest), so the first n_live sorted places are exactly the live rows.
__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_key_kernel(const float* __restrict__ pts, int64_t n_cap,
                                                                const int32_t* __restrict__ n_dev, double vs, CloudBox* box,
                                                                uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t n = live_rows(n_cap, n_dev);
  const bool bad = (box->flags & CNRMA_CLOUD_NONFINITE) != 0;
  double org[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) org[a] = (double)f32_from_ordered(box->lo[a]) - 0.5 * vs;
  bool wide = false;
  for (int64_t i = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; i < n_cap; i += (int64_t)gridDim.x * CLOUD_BLOCK) {
    uint64_t key = ~0ull;
    if (i < n && !bad) {
      uint64_t k[3];
      bool fits = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double f = floor(((double)pts[i * 3 + a] - org[a]) / vs);
        fits = fits && f >= 0.0 && f < (double)(1 << CLOUD_KEY_BITS);
        k[a] = fits ? (uint64_t)f : 0;
      }
      if (fits) key = (k[0] << (2 * CLOUD_KEY_BITS)) | (k[1] << CLOUD_KEY_BITS) | k[2];
      else wide = true;
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
  }
  if (__ballot(wide) != 0 && (threadIdx.x & 63) == 0) atomicOr(&box->flags, CNRMA_CLOUD_VOXEL_TOO_SMALL);
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_head_kernel(const uint64_t* __restrict__ keys, int64_t n_cap,
                                                                 const int32_t* __restrict__ n_dev, int32_t* __restrict__ head) {
  const int64_t n = live_rows(n_cap, n_dev);
  for (int64_t j = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; j < n_cap; j += (int64_t)gridDim.x * CLOUD_BLOCK)
    head[j] = (j < n && (j == 0 || keys[j] != keys[j - 1])) ? 1 : 0;
}

// one thread per voxel: the fp64 sums of its points in sorted order = ascending input index
__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_mean_kernel(const float* __restrict__ pts, int64_t n_cap,
                                                                 const int32_t* __restrict__ n_dev, const CloudBox* box,
                                                                 const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                                 const int32_t* __restrict__ head, const int32_t* __restrict__ off,
                                                                 float* __restrict__ out_points, int32_t* __restrict__ out_count,
                                                                 int64_t out_cap, int32_t* __restrict__ info) {
  const int64_t n = live_rows(n_cap, n_dev);
  const int flags = box->flags;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    info[0] = flags ? 0 : off[n_cap];
    info[1] = flags;
    info[2] = 0;
    info[3] = 0;
  }
  if (flags) return;
  for (int64_t j = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * CLOUD_BLOCK) {
    if (!head[j]) continue;
    const int64_t v = off[j];
    if (v >= out_cap) continue;
    const uint64_t key = keys[j];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int32_t c = 0;
    for (int64_t e = j; e < n && keys[e] == key; ++e) {
      const int64_t i = vals[e];
      sx += (double)pts[i * 3];
      sy += (double)pts[i * 3 + 1];
      sz += (double)pts[i * 3 + 2];
      ++c;
    }
    const double d = (double)c;
    out_points[v * 3] = (float)(sx / d);
    out_points[v * 3 + 1] = (float)(sy / d);
    out_points[v * 3 + 2] = (float)(sz / d);
    if (out_count != nullptr) out_count[v] = c;
  }
}

__global__ void cloud_info_zero_kernel(int32_t* info) {
  if (threadIdx.x < 4) info[threadIdx.x] = 0;
}

// ================================================================================================================
// exact nearest neighbour
// ================================================================================================================
struct NnHeader {             // written by one thread of the build, read by every query
  double o[3];                // the grid's origin = the targets' fp32 minimum
  double h;                   // cell size
  int32_t dim[3];
  int32_t n_cells;
  int32_t n_live;             // live (finite or not) targets
  int32_t pad[3];
};
static_assert(sizeof(NnHeader) == 64, "the header has a fixed place in the workspace");

struct NnLayout {
  size_t header, box, part, key_a, key_b, val_a, val_b, rec, start, sort_tmp, sort_tmp_bytes, total;
};

NnLayout nn_layout(int64_t n) {
  NnLayout L{};
  const size_t n4 = (size_t)((n + 3) / 4 * 4);
  size_t p = 0;
  L.header = p; p += 64;
  L.box = p; p += 192;
  L.part = p; p += align256((CLOUD_SCAN_BLOCKS + 1) * sizeof(int32_t));
  L.key_a = p; p += align256(n4 * 4);
  L.key_b = p; p += align256(n4 * 4);
  L.val_a = p; p += align256(n4 * 4);
  L.val_b = p; p += align256(n4 * 4);
  L.rec = p; p += align256(n4 * 16);
  L.start = p; p += align256((size_t)(CLOUD_MAX_CELLS + CLOUD_SCAN_TILE) * sizeof(int32_t));
  L.sort_tmp_bytes = cloud_sort_temp_bytes<uint32_t>(n > 0 ? n : 1);
  L.sort_tmp = p; p += L.sort_tmp_bytes;
  L.total = p;
  return L;
}

// cell of a coordinate along one axis, clamped into the grid (NaN -> 0)
__device__ __forceinline__ int nn_cell(double p, double o, double h, int dim) {
  const double f = floor((p - o) / h);
  if (!(f > 0.0)) return 0;
  return f >= (double)dim ? dim - 1 : (int)f;
}

__global__ void cloud_nn_header_kernel(const CloudBox* box, int64_t n_cap, const int32_t* n_dev, double cell, NnHeader* H) {
  const int64_t n = live_rows(n_cap, n_dev);
  double e[3];
  bool ok = n > 0 && box->flags == 0 && box->lo[0] != 0xffffffffu;
  for (int a = 0; a < 3; ++a) {
    const double lo = ok ? (double)f32_from_ordered(box->lo[a]) : 0.0, hi = ok ? (double)f32_from_ordered(box->hi[a]) : 0.0;
    H->o[a] = lo;
    e[a] = hi - lo;
  }
  // a grid of one cell is always exact (a plain scan over all targets): the shape for no targets and for non-finite ones
  double h = cell, d[3] = {1.0, 1.0, 1.0};
  if (ok) {
    for (int it = 0; it < 4096; ++it) {
      for (int a = 0; a < 3; ++a) d[a] = floor(e[a] / h) + 1.0;
      if (d[0] * d[1] * d[2] <= (double)CLOUD_MAX_CELLS) break;
      h *= 1.125;
    }
    if (!(d[0] * d[1] * d[2] <= (double)CLOUD_MAX_CELLS)) d[0] = d[1] = d[2] = 1.0;
  }
  H->h = h;
  for (int a = 0; a < 3; ++a) H->dim[a] = (int32_t)d[a];
  H->n_cells = H->dim[0] * H->dim[1] * H->dim[2];
  H->n_live = (int32_t)n;
  H->pad[0] = H->pad[1] = H->pad[2] = 0;
}

// clears the live part of the starts: n_cells + 1 words
__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_clear_kernel(const NnHeader* H, int32_t* __restrict__ start) {
  const int n = H->n_cells + 1;
  for (int c = blockIdx.x * CLOUD_BLOCK + threadIdx.x; c < n; c += gridDim.x * CLOUD_BLOCK) start[c] = 0;
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_cell_kernel(const float* __restrict__ pts, int64_t n_cap, const NnHeader* H,
                                                              uint32_t* __restrict__ keys, int32_t* __restrict__ vals,
                                                              int32_t* __restrict__ start) {
  const int64_t n = H->n_live;
  const double ox = H->o[0], oy = H->o[1], oz = H->o[2], h = H->h;
  const int dx = H->dim[0], dy = H->dim[1], dz = H->dim[2];
  for (int64_t i = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; i < n_cap; i += (int64_t)gridDim.x * CLOUD_BLOCK) {
    uint32_t key = (uint32_t)CLOUD_MAX_CELLS;                      // dead rows sort last (bit 24)
    if (i < n) {
      const int cx = nn_cell((double)pts[i * 3], ox, h, dx), cy = nn_cell((double)pts[i * 3 + 1], oy, h, dy),
                cz = nn_cell((double)pts[i * 3 + 2], oz, h, dz);
      key = (uint32_t)((cx * dy + cy) * dz + cz);
      atomicAdd(&start[key], 1);
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
  }
}

// exclusive scan of start[0 .. n_cells] in place, the count read on the device: chunk sums, a scan of the chunk sums, then every
// block scans its chunk tile by tile
__device__ __forceinline__ void nn_chunk(const NnHeader* H, int* c0, int* c1) {
  const int n = H->n_cells + 1;
  int per = (n + CLOUD_SCAN_BLOCKS - 1) / CLOUD_SCAN_BLOCKS;
  per = (per + CLOUD_SCAN_TILE - 1) / CLOUD_SCAN_TILE * CLOUD_SCAN_TILE;
  const int64_t b0 = (int64_t)blockIdx.x * per;
  *c0 = (int)(b0 < n ? b0 : n);
  *c1 = (int)(b0 + per < n ? b0 + per : n);
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_scan_sum_kernel(const NnHeader* H, const int32_t* __restrict__ start,
                                                                  int32_t* __restrict__ part) {
  __shared__ int smem[CLOUD_BLOCK / 64 + 1];
  int c0, c1;
  nn_chunk(H, &c0, &c1);
  int s = 0;
  for (int c = c0 + threadIdx.x; c < c1; c += CLOUD_BLOCK) s += start[c];
  int total;
  (void)block_excl_scan<CLOUD_BLOCK>(s, smem, &total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(CLOUD_SCAN_BLOCKS) void cloud_nn_scan_part_kernel(int32_t* __restrict__ part) {
  __shared__ int smem[CLOUD_SCAN_BLOCKS / 64 + 1];
  int total;
  const int v = part[threadIdx.x];
  const int e = block_excl_scan<CLOUD_SCAN_BLOCKS>(v, smem, &total);
  part[threadIdx.x] = e;
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_scan_apply_kernel(const NnHeader* H, int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ part) {
  __shared__ int smem[CLOUD_BLOCK / 64 + 1];
  int c0, c1;
  nn_chunk(H, &c0, &c1);
  int base = part[blockIdx.x];
  for (int t0 = c0; t0 < c1; t0 += CLOUD_SCAN_TILE) {            // block-uniform
    const int c = t0 + (int)threadIdx.x * 4;
    int v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < c1 ? start[c + k] : 0;
    const int s = (v[0] + v[1]) + (v[2] + v[3]);
    int total;
    int e = base + block_excl_scan<CLOUD_BLOCK>(s, smem, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c + k < c1) start[c + k] = e;
      e += v[k];
    }
    base += total;
  }
}

__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_record_kernel(const float* __restrict__ pts, const NnHeader* H,
                                                                const int32_t* __restrict__ vals, float4* __restrict__ rec) {
  const int64_t n = H->n_live;
  for (int64_t j = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * CLOUD_BLOCK) {
    const int32_t i = vals[j];
    rec[j] = make_float4(pts[(int64_t)i * 3], pts[(int64_t)i * 3 + 1], pts[(int64_t)i * 3 + 2], __int_as_float(i));
  }
}

struct NnBest { double d2; int32_t idx; };

__device__ __forceinline__ void nn_scan_range(const float4* __restrict__ rec, int b, int e, double qx, double qy, double qz,
                                              NnBest* best) {
  for (int j = b; j < e; ++j) {
    const float4 t = rec[j];
    const double dx = qx - (double)t.x, dy = qy - (double)t.y, dz = qz - (double)t.z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const int32_t i = __float_as_int(t.w);
    if (d2 < best->d2 || (d2 == best->d2 && i < best->idx)) { best->d2 = d2; best->idx = i; }
  }
}

// distance from q to the two faces of the visited block along one axis that are not the grid's boundary, less the margin
__device__ __forceinline__ double nn_axis_bound(double q, double o, double h, int c, int r, int dim, double bound, bool* open) {
  if (c - r > 0) {
    const double face = o + (double)(c - r) * h;
    bound = fmin(bound, (q - face) - (1e-6 * h + 1e-13 * (fabs(q) + fabs(face))));
    *open = true;
  }
  if (c + r < dim - 1) {
    const double face = o + (double)(c + r + 1) * h;
    bound = fmin(bound, (face - q) - (1e-6 * h + 1e-13 * (fabs(q) + fabs(face))));
    *open = true;
  }
  return bound;
}

template <bool STATS>
__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_nn_query_kernel(const float* __restrict__ qs, int64_t nq_cap,
                                                               const int32_t* __restrict__ nq_dev, const NnHeader* H,
                                                               const float4* __restrict__ rec, const int32_t* __restrict__ start,
                                                               double* __restrict__ dist, int32_t* __restrict__ idx,
                                                               unsigned long long* __restrict__ stats) {
  const int64_t nq = live_rows(nq_cap, nq_dev);
  const int64_t q = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x;
  if (q >= nq) return;
  const double qx = (double)qs[q * 3], qy = (double)qs[q * 3 + 1], qz = (double)qs[q * 3 + 2];
  const double ox = H->o[0], oy = H->o[1], oz = H->o[2], h = H->h;
  const int dx = H->dim[0], dy = H->dim[1], dz = H->dim[2];
  const int cx = nn_cell(qx, ox, h, dx), cy = nn_cell(qy, oy, h, dy), cz = nn_cell(qz, oz, h, dz);
  NnBest best{INFINITY, -1};
  unsigned long long shells = 0, cands = 0;
  if (H->n_live > 0) {
    for (int r = 0;; ++r) {
      const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
      const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
      for (int x = x0; x <= x1; ++x) {
        const bool x_face = x == cx - r || x == cx + r;
        for (int y = y0; y <= y1; ++y) {
          const int row = (x * dy + y) * dz;
          if (x_face || y == cy - r || y == cy + r) {             // the row's whole z range belongs to the shell
            const int b = start[row + z0], e = start[row + z1 + 1];
            nn_scan_range(rec, b, e, qx, qy, qz, &best);
            if (STATS) cands += (unsigned long long)(e - b);
          } else {                                                // its two end cells, where they exist
            if (cz - r >= 0) {
              const int b = start[row + cz - r], e = start[row + cz - r + 1];
              nn_scan_range(rec, b, e, qx, qy, qz, &best);
              if (STATS) cands += (unsigned long long)(e - b);
            }
            if (cz + r < dz) {
              const int b = start[row + cz + r], e = start[row + cz + r + 1];
              nn_scan_range(rec, b, e, qx, qy, qz, &best);
              if (STATS) cands += (unsigned long long)(e - b);
            }
          }
        }
      }
      if (STATS) ++shells;
      bool open = false;
      double bound = INFINITY;
      bound = nn_axis_bound(qx, ox, h, cx, r, dx, bound, &open);
      bound = nn_axis_bound(qy, oy, h, cy, r, dy, bound, &open);
      bound = nn_axis_bound(qz, oz, h, cz, r, dz, bound, &open);
      if (!open) break;                                           // the block covers the grid
      if (bound > 0.0 && best.d2 < bound * bound) break;          // strictly: an equal distance with a lower index may be outside
    }
  }
  dist[q] = sqrt(best.d2);
  idx[q] = best.idx;
  if (STATS) {
    atomicAdd(&stats[0], shells);
    atomicAdd(&stats[1], cands);
  }
}

// ================================================================================================================
// scores
// ================================================================================================================
__global__ __launch_bounds__(CLOUD_BLOCK) void cloud_score_kernel(const double* __restrict__ dist, int64_t n_cap,
                                                                  const int32_t* __restrict__ n_dev, double thr,
                                                                  double* __restrict__ d_live, double* __restrict__ below,
                                                                  double* __restrict__ out) {
  const int64_t n = live_rows(n_cap, n_dev);
  if (blockIdx.x == 0 && threadIdx.x == 0) out[2] = (double)n;
  for (int64_t i = (int64_t)blockIdx.x * CLOUD_BLOCK + threadIdx.x; i < n_cap; i += (int64_t)gridDim.x * CLOUD_BLOCK) {
    const bool live = i < n;
    const double d = live ? dist[i] : 0.0;
    d_live[i] = d;
    below[i] = (live && d < thr) ? 1.0 : 0.0;
  }
}

bool cloud_rows_ok(int64_t n) { return n >= 0 && n <= CLOUD_MAX_POINTS; }

}  // namespace

extern "C" size_t cnrma_cloud_downsample_workspace_bytes(int64_t n_cap) {
  if (!cloud_rows_ok(n_cap)) return 0;
  return down_layout(n_cap).total;
}

extern "C" int cnrma_cloud_voxel_downsample_f32(const float* points, int64_t n_cap, const int32_t* n_dev, double voxel_size,
                                                void* workspace, size_t workspace_bytes, float* out_points, int32_t* out_count,
                                                int64_t out_cap, int32_t* info, void* stream) {
  if (!cloud_rows_ok(n_cap) || !(voxel_size > 0.0) || !isfinite(voxel_size) || info == nullptr || out_cap < 0 ||
      (out_cap > 0 && out_points == nullptr))
    return CNRMA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (n_cap == 0) {
    hipLaunchKernelGGL(cloud_info_zero_kernel, dim3(1), dim3(64), 0, st, info);
    CNRMA_LAUNCH_CHECK();
    return 0;
  }
  const DownLayout L = down_layout(n_cap);
  if (points == nullptr || workspace == nullptr || workspace_bytes < L.total || ((uintptr_t)workspace & 15) != 0) return CNRMA_EINVAL;
  char* ws = static_cast<char*>(workspace);
  CloudBox* box = reinterpret_cast<CloudBox*>(ws + L.box);
  uint64_t* key_a = reinterpret_cast<uint64_t*>(ws + L.key_a);
  uint64_t* key_b = reinterpret_cast<uint64_t*>(ws + L.key_b);
  int32_t* val_a = reinterpret_cast<int32_t*>(ws + L.val_a);
  int32_t* val_b = reinterpret_cast<int32_t*>(ws + L.val_b);
  int32_t* head = reinterpret_cast<int32_t*>(ws + L.head);
  int32_t* off = reinterpret_cast<int32_t*>(ws + L.off);
  const dim3 grid(cloud_grid(n_cap)), block(CLOUD_BLOCK);
  hipLaunchKernelGGL(cloud_box_init_kernel, dim3(1), dim3(1), 0, st, box);
  hipLaunchKernelGGL(cloud_box_kernel, dim3(cloud_grid(n_cap, CLOUD_BOX_BLOCKS)), block, 0, st, points, n_cap, n_dev, box);
  hipLaunchKernelGGL(cloud_key_kernel, grid, block, 0, st, points, n_cap, n_dev, voxel_size, box, key_a, val_a);
  size_t tmp = L.sort_tmp_bytes;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(ws + L.sort_tmp, tmp, key_a, key_b, val_a, val_b, (int)n_cap, 0, 64, st);
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL(cloud_head_kernel, grid, block, 0, st, key_b, n_cap, n_dev, head);
  int rc = cnrma_exclusive_scan_i32(head, off, n_cap, ws + L.scan, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(cloud_mean_kernel, grid, block, 0, st, points, n_cap, n_dev, box, key_b, val_b, head, off, out_points,
                     out_count, out_cap, info);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cnrma_cloud_nn_workspace_bytes(int64_t n_cap) {
  if (!cloud_rows_ok(n_cap)) return 0;
  return nn_layout(n_cap).total;
}

extern "C" int cnrma_cloud_nn_build_f32(const float* targets, int64_t n_cap, const int32_t* n_dev, double cell, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  if (!cloud_rows_ok(n_cap) || !(cell > 0.0) || !isfinite(cell) || workspace == nullptr || (n_cap > 0 && targets == nullptr))
    return CNRMA_EINVAL;
  const NnLayout L = nn_layout(n_cap);
  if (workspace_bytes < L.total || ((uintptr_t)workspace & 15) != 0) return CNRMA_EINVAL;
  char* ws = static_cast<char*>(workspace);
  NnHeader* H = reinterpret_cast<NnHeader*>(ws + L.header);
  CloudBox* box = reinterpret_cast<CloudBox*>(ws + L.box);
  int32_t* part = reinterpret_cast<int32_t*>(ws + L.part);
  uint32_t* key_a = reinterpret_cast<uint32_t*>(ws + L.key_a);
  uint32_t* key_b = reinterpret_cast<uint32_t*>(ws + L.key_b);
  int32_t* val_a = reinterpret_cast<int32_t*>(ws + L.val_a);
  int32_t* val_b = reinterpret_cast<int32_t*>(ws + L.val_b);
  float4* rec = reinterpret_cast<float4*>(ws + L.rec);
  int32_t* start = reinterpret_cast<int32_t*>(ws + L.start);
  hipStream_t st = as_stream(stream);
  const dim3 grid(cloud_grid(n_cap)), block(CLOUD_BLOCK);
  hipLaunchKernelGGL(cloud_box_init_kernel, dim3(1), dim3(1), 0, st, box);
  if (n_cap > 0)
    hipLaunchKernelGGL(cloud_box_kernel, dim3(cloud_grid(n_cap, CLOUD_BOX_BLOCKS)), block, 0, st, targets, n_cap, n_dev, box);
  hipLaunchKernelGGL(cloud_nn_header_kernel, dim3(1), dim3(1), 0, st, box, n_cap, n_dev, cell, H);
  hipLaunchKernelGGL(cloud_nn_clear_kernel, dim3(2048), block, 0, st, H, start);
  if (n_cap > 0) {
    hipLaunchKernelGGL(cloud_nn_cell_kernel, grid, block, 0, st, targets, n_cap, H, key_a, val_a, start);
    size_t tmp = L.sort_tmp_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(ws + L.sort_tmp, tmp, key_a, key_b, val_a, val_b, (int)n_cap, 0, 25, st);
    if (e != hipSuccess) return -(int)e;
  }
  hipLaunchKernelGGL(cloud_nn_scan_sum_kernel, dim3(CLOUD_SCAN_BLOCKS), block, 0, st, H, start, part);
  hipLaunchKernelGGL(cloud_nn_scan_part_kernel, dim3(1), dim3(CLOUD_SCAN_BLOCKS), 0, st, part);
  hipLaunchKernelGGL(cloud_nn_scan_apply_kernel, dim3(CLOUD_SCAN_BLOCKS), block, 0, st, H, start, part);
  if (n_cap > 0) hipLaunchKernelGGL(cloud_nn_record_kernel, grid, block, 0, st, targets, H, val_b, rec);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_cloud_nn_query_f32(const float* queries, int64_t nq_cap, const int32_t* nq_dev, int64_t nt_cap,
                                        const void* workspace, double* dist, int32_t* idx, uint64_t* stats, void* stream) {
  if (!cloud_rows_ok(nq_cap) || !cloud_rows_ok(nt_cap) || workspace == nullptr || ((uintptr_t)workspace & 15) != 0)
    return CNRMA_EINVAL;
  if (nq_cap == 0) return 0;
  if (queries == nullptr || dist == nullptr || idx == nullptr) return CNRMA_EINVAL;
  const NnLayout L = nn_layout(nt_cap);
  const char* ws = static_cast<const char*>(workspace);
  const NnHeader* H = reinterpret_cast<const NnHeader*>(ws + L.header);
  const float4* rec = reinterpret_cast<const float4*>(ws + L.rec);
  const int32_t* start = reinterpret_cast<const int32_t*>(ws + L.start);
  const dim3 grid((unsigned)ceil_div(nq_cap, CLOUD_BLOCK)), block(CLOUD_BLOCK);
  unsigned long long* s = reinterpret_cast<unsigned long long*>(stats);
  if (stats != nullptr)
    hipLaunchKernelGGL(cloud_nn_query_kernel<true>, grid, block, 0, as_stream(stream), queries, nq_cap, nq_dev, H, rec, start, dist, idx, s);
  else
    hipLaunchKernelGGL(cloud_nn_query_kernel<false>, grid, block, 0, as_stream(stream), queries, nq_cap, nq_dev, H, rec, start, dist, idx, s);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cnrma_cloud_score_workspace_bytes(int64_t n_cap) {
  if (!cloud_rows_ok(n_cap)) return 0;
  return 2 * align256((size_t)(n_cap > 0 ? n_cap : 1) * sizeof(double)) + align256(cnrma_scan_workspace_bytes(n_cap > 0 ? n_cap : 1));
}

extern "C" int cnrma_cloud_score_f64(const double* dist, int64_t n_cap, const int32_t* n_dev, double threshold, void* workspace,
                                     size_t workspace_bytes, double* out3, void* stream) {
  if (!cloud_rows_ok(n_cap) || workspace == nullptr || out3 == nullptr || (n_cap > 0 && dist == nullptr) ||
      workspace_bytes < cnrma_cloud_score_workspace_bytes(n_cap) || ((uintptr_t)workspace & 15) != 0)
    return CNRMA_EINVAL;
  char* ws = static_cast<char*>(workspace);
  const size_t stride = align256((size_t)(n_cap > 0 ? n_cap : 1) * sizeof(double));
  double* d_live = reinterpret_cast<double*>(ws);
  double* below = reinterpret_cast<double*>(ws + stride);
  void* sum_ws = ws + 2 * stride;
  hipLaunchKernelGGL(cloud_score_kernel, dim3(cloud_grid(n_cap)), dim3(CLOUD_BLOCK), 0, as_stream(stream), dist, n_cap, n_dev,
                     threshold, d_live, below, out3);
  int rc = cnrma_sum_f64(d_live, out3, n_cap, sum_ws, stream);
  if (rc == 0) rc = cnrma_sum_f64(below, out3 + 1, n_cap, sum_ws, stream);
  if (rc != 0) return rc;
  CNRMA_LAUNCH_CHECK();
  return 0;
}
