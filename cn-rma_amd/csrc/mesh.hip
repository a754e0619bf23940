// Mesh extraction from a TSDF volume: marching cubes on the device (reference: datasets/tsdf.py:81-114, TSDF.get_mesh, which
// calls scikit-image on the host).  The conventions -- corner / edge numbering, the face rule that makes neighbouring cells
// agree, loop orientation, fan triangulation -- are those of cnrma_amd/mesh_table.py, which generates mesh_table.inc.
//
//   field     g = (v == 1) ? 1 : clamp(-v, -1, 1), fused into every load (tsdf.py:95-104); "inside" is g > 0
//   vertices  a voxel OWNS the three edges that leave it in +x, +y, +z; an owned edge with a sign change is one vertex, so vertices
//             are welded by construction.  Order: the owner's linear index (x Y + y) Z + z, then the axis
//   faces     a cell contributes the triangles of its case.  Order: the cell's linear index, then table order
//
// count:  classify (a wave per run of 16 x 64 voxels: per 64 voxels the ballots of owned edges, of list membership and of the
//         triangle counts, per run their totals and the sign flags; ballot + popcount, no atomics)  ->  scan of the run totals
//         (one block)  ->  compact (from the ballots alone: the first vertex number of every 64 voxels, and the compacted list of
//         voxels that own a vertex or an active cell)
// emit:   one thread per list entry: its <= 3 vertices + normals and its cell's <= 5 triangles; a vertex number anywhere in the
//         volume is its chunk's first number + popcounts of the chunk's ballots below the owner's lane -- no per-voxel offset array
//
// Lanes run along z (the linear index), so the four row loads of a wave (x / x+1, y / y+1) coalesce and the z+1 corners come from
// the next lane's sign bits (one shuffle; lane 63 takes them from the wave's next chunk).  Rows are re-read through L1 / L2 rather
// than staged in LDS: each row is used by four waves, the kernel has no other reuse, and without a tile there is no barrier in the
// loads' way.  No tuning state, nothing read from the environment, no allocation and no synchronisation inside.
#include "common.h"
#include "mesh_table.inc"

namespace {

constexpr int MESH_BLOCK = 256;
constexpr int MESH_RUN = 16;         // 64-voxel chunks per wave of the classify and compact kernels ...
constexpr int MESH_BATCH = 8;        // ... loaded this many at a time
constexpr int64_t MESH_MAX_VOXELS = (int64_t)1 << 28;      // 5 triangles / 3 vertices per voxel and every index stay inside int32

struct MeshWave {                 // per 64 consecutive voxels (a "chunk")
  unsigned long long bx, by, bz;  // lanes whose +x / +y / +z edge carries a vertex
  int32_t v_first;                // number of the chunk's first vertex (written by the compaction)
  int32_t pad;
  unsigned long long bl;          // lanes on the list: they own a vertex or an active cell
  unsigned long long t0, t1, t2;  // bits 0 / 1 / 2 of the lanes' triangle counts
};
static_assert(sizeof(MeshWave) == 64, "the emit kernel reads the first half of a MeshWave as two 16-byte words");

struct MeshLayout {
  size_t header, run_tot, run_off, waves, list, total;
  int64_t n, n_runs, n_waves;
};

MeshLayout mesh_layout(int X, int Y, int Z) {
  MeshLayout L{};
  L.n = (int64_t)X * Y * Z;
  L.n_runs = ceil_div(L.n, MESH_RUN * 64);
  L.n_waves = ceil_div(L.n, 64);
  L.header = 0;
  L.run_tot = 64;
  L.run_off = L.run_tot + (size_t)L.n_runs * sizeof(int4);
  L.waves = L.run_off + (size_t)L.n_runs * sizeof(int4);
  L.list = L.waves + (size_t)L.n_waves * sizeof(MeshWave);
  L.total = L.list + (size_t)L.n * sizeof(int2);           // worst case: every voxel on the list
  return L;
}

bool mesh_dims_ok(int X, int Y, int Z) { return X > 0 && Y > 0 && Z > 0 && (int64_t)X * Y * Z <= MESH_MAX_VOXELS; }

__device__ __forceinline__ float mesh_field(float v) { return v == 1.0f ? 1.0f : fminf(fmaxf(-v, -1.0f), 1.0f); }

// One 64-voxel chunk as a wave loads it: per lane the four rows (x / x+1, y / y+1) at the lane's z, and which neighbours exist.
// The loads are unconditional, from indices clamped into the volume: a value whose voxel does not exist is never looked at (an
// edge needs its `has` bit, a cell all three), and a branch per guarded load costs more than the load.
struct MeshChunk {
  float v00, v10, v01, v11;   // tsdf at (x + dx, y + dy, z)
  int has;                    // bit 0 / 1 / 2: x + 1 < X, y + 1 < Y, z + 1 < Z; bit 3: the voxel itself exists
};

// g > 0 <=> v < 0 or v == 1 (the clamp keeps the sign; NaN is outside);  g < 0 <=> v > 0 and v != 1
__device__ __forceinline__ bool mesh_inside(float v) { return v < 0.0f || v == 1.0f; }
__device__ __forceinline__ int mesh_nib(const MeshChunk& c) {          // bit dx + 2 dy: g > 0 at (x + dx, y + dy, z)
  return (int)mesh_inside(c.v00) | ((int)mesh_inside(c.v10) << 1) | ((int)mesh_inside(c.v01) << 2) | ((int)mesh_inside(c.v11) << 3);
}

// voxel i = (x, y, z); x + 1 < X <=> i + YZ < n
__device__ __forceinline__ MeshChunk mesh_load_chunk(const float* __restrict__ tsdf, int i, int n, int y, int z, int Y, int Z,
                                                     int YZ) {
  const int last = n - 1;
  MeshChunk c;
  c.v00 = tsdf[min(i, last)];
  c.v10 = tsdf[min(i + YZ, last)];
  c.v01 = tsdf[min(i + Z, last)];
  c.v11 = tsdf[min(i + YZ + Z, last)];
  const bool valid = i < n;
  c.has = (int)(i + YZ < n) | ((int)(valid && y + 1 < Y) << 1) | ((int)(valid && z + 1 < Z) << 2) | ((int)valid << 3);
  return c;
}

// A wave walks MESH_RUN consecutive 64-voxel chunks (a "run"), MESH_BATCH at a time: the loads of a whole batch and of the chunk
// behind it are issued before the first is used.  The z + 1 corners of a chunk are the next lane's bits; lane 63 takes them from
// lane 0 of the NEXT chunk (the one extra chunk of loads at the end of a batch).
// Writes per chunk its MeshWave (all but v_first) and per run the totals {vertices, triangles, active cells, list entries | sign
// flags << 16}; the volume is read here and by the emit only.
// SMALL_Z: Z < 64, where 64 voxels further along can be several rows on (a division per chunk instead of one wrap)
template <bool SMALL_Z>
__global__ __launch_bounds__(MESH_BLOCK) void mesh_classify_kernel(const float* __restrict__ tsdf, int Y, int Z, int n,
                                                                   int4* __restrict__ run_tot, MeshWave* __restrict__ waves) {
  __shared__ unsigned char s_ntri[256];
  s_ntri[threadIdx.x] = MESH_NTRI[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int run = __builtin_amdgcn_readfirstlane(blockIdx.x * (MESH_BLOCK / 64) + (threadIdx.x >> 6));
  const int first = run * (MESH_RUN * 64);
  if (first >= n) return;                                   // whole waves only; no block-wide step follows
  const int YZ = Y * Z;
  int i = first + lane;                                     // may pass n in the last chunks: (y, z) stay consistent, `has` is 0
  int y, z;
  {
    const int r = i % YZ;
    y = r / Z;
    z = r - y * Z;
  }
  int4 acc = make_int4(0, 0, 0, 0);
  int flags = 0;
  for (int batch = 0; batch < MESH_RUN / MESH_BATCH; ++batch) {
    if (first + batch * (MESH_BATCH * 64) >= n) break;      // wave-uniform
    MeshChunk ch[MESH_BATCH + 1];
    int yb = y, zb = z;                                     // (y, z) of voxel i; the batch's last + 1 chunk starts the next batch
#pragma unroll
    for (int c = 0; c <= MESH_BATCH; ++c) {
      ch[c] = mesh_load_chunk(tsdf, i + c * 64, n, yb, zb, Y, Z, YZ);
      if (c == MESH_BATCH) break;
      zb += 64;
      if (SMALL_Z) {
        const int q = zb / Z;
        zb -= q * Z;
        yb = (yb + q) % Y;
      } else if (zb >= Z) {                                 // Z >= 64: one row further at most
        zb -= Z;
        yb = yb + 1 == Y ? 0 : yb + 1;
      }
    }
    y = yb; z = zb;
    int nib = mesh_nib(ch[0]);
#pragma unroll
    for (int c = 0; c < MESH_BATCH; ++c) {
      const int i0 = i + c * 64;
      const int nib_next = mesh_nib(ch[c + 1]);
      int nibz = __shfl_down(nib, 1, 64);                   // the lane above is z + 1 of the same (x, y) whenever that exists
      const int next_first = __builtin_amdgcn_readlane(nib_next, 0);
      if (lane == 63) nibz = next_first;
      const int cs = nib | (nibz << 4);
      const int has = ch[c].has;
      const bool active = (has & 7) == 7 && cs != 0 && cs != 255;
      const int b0 = nib & 1;
      const bool ex = (has & 1) && b0 != ((nib >> 1) & 1), ey = (has & 2) && b0 != ((nib >> 2) & 1), ez = (has & 4) && b0 != (nibz & 1);
      const int nt = active ? (int)s_ntri[cs] : 0;
      const unsigned long long bx = __ballot(ex), by = __ballot(ey), bz = __ballot(ez);
      const unsigned long long bl = __ballot(ex || ey || ez || active);
      const unsigned long long t0 = __ballot(nt & 1), t1 = __ballot(nt & 2), t2 = __ballot(nt & 4);
      acc.z += __popcll(__ballot(active));
      const float v = ch[c].v00;
      flags |= (__ballot((has & 8) && v > 0.0f && v != 1.0f) != 0 ? 1 : 0) | (__ballot((has & 8) && (nib & 1)) != 0 ? 2 : 0);
      if (lane == 0 && i0 < n) {
        MeshWave W;
        W.bx = bx; W.by = by; W.bz = bz; W.v_first = 0; W.pad = 0;
        W.bl = bl; W.t0 = t0; W.t1 = t1; W.t2 = t2;
        waves[i0 >> 6] = W;
      }
      acc.x += __popcll(bx) + __popcll(by) + __popcll(bz);
      acc.y += __popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2);
      acc.w += __popcll(bl);
      nib = nib_next;
    }
    i += MESH_BATCH * 64;
  }
  if (lane == 0) {
    acc.w |= flags << 16;                                   // at most MESH_RUN * 64 list entries: far below 2^16
    run_tot[run] = acc;
  }
}

__device__ __forceinline__ unsigned long long mesh_readlane64(unsigned long long v, int src) {      // src wave-uniform
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// The compaction, from the chunks' masks alone (the volume is not read again): a wave takes a run; lane c loads chunk c's masks,
// a wave scan of their popcounts gives every chunk its first vertex / triangle / list position, and the chunks' list entries
// {voxel, number of its cell's first triangle} are then written chunk by chunk with the masks passed from lane c
__global__ __launch_bounds__(MESH_BLOCK) void mesh_compact_kernel(int n, const int4* __restrict__ run_off, MeshWave* waves,
                                                                  int2* __restrict__ list) {
  static_assert(MESH_RUN <= 64, "one lane per chunk of a run");
  const int lane = threadIdx.x & 63;
  const int run = __builtin_amdgcn_readfirstlane(blockIdx.x * (MESH_BLOCK / 64) + (threadIdx.x >> 6));
  const int first = run * (MESH_RUN * 64);
  if (first >= n) return;
  const int left = (n - first + 63) >> 6, n_chunks = left < MESH_RUN ? left : MESH_RUN;      // wave-uniform
  const int4 base = run_off[run];
  MeshWave* W = waves + (first >> 6) + lane;                // this lane's chunk, when lane < n_chunks
  unsigned long long bl = 0, t0 = 0, t1 = 0, t2 = 0;
  int sv = 0;
  if (lane < n_chunks) {
    sv = __popcll(W->bx) + __popcll(W->by) + __popcll(W->bz);
    bl = W->bl; t0 = W->t0; t1 = W->t1; t2 = W->t2;
  }
  const int st = __popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2), sl = __popcll(bl);
  const int v_first = base.x + wave_incl_scan(sv) - sv;
  const int t_first = base.y + wave_incl_scan(st) - st;
  const int l_first = base.w + wave_incl_scan(sl) - sl;
  if (lane < n_chunks) W->v_first = v_first;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c = 0; c < n_chunks; ++c) {
    const unsigned long long cl = mesh_readlane64(bl, c);
    if (cl == 0) continue;                                  // wave-uniform: most chunks lie in empty space
    const unsigned long long c0 = mesh_readlane64(t0, c), c1 = mesh_readlane64(t1, c), c2 = mesh_readlane64(t2, c);
    const int tb = __builtin_amdgcn_readlane(t_first, c), lb = __builtin_amdgcn_readlane(l_first, c);
    if ((cl >> lane) & 1ull)
      list[lb + __popcll(cl & below)] = make_int2(first + c * 64 + lane,                      // < the list's total <= n
                                                  tb + __popcll(c0 & below) + 2 * __popcll(c1 & below) + 4 * __popcll(c2 & below));
  }
}

// exclusive offsets of the run totals (one block; every thread takes a stretch of consecutive runs, loaded eight at a time so that
// the loads overlap), the counts, and the reference's empty rule (tsdf.py:106-107): no g < 0 or no g > 0 -> an empty mesh
__global__ __launch_bounds__(1024) void mesh_scan_kernel(const int4* __restrict__ run_tot, int4* __restrict__ run_off, int n_runs,
                                                         int no_cells, int32_t* __restrict__ counts, int32_t* __restrict__ header) {
  __shared__ int smem[1024 / 64 + 1];
  const int per = (n_runs + 1023) / 1024;
  const int b0 = min(n_runs, (int)threadIdx.x * per), b1 = min(n_runs, b0 + per);
  int sv = 0, st = 0, sc = 0, sl = 0, flags = 0;
  for (int b = b0; b < b1; b += 8) {
    int4 t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = b + j < b1 ? run_tot[b + j] : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sv += t[j].x; st += t[j].y; sc += t[j].z; sl += t[j].w & 0xffff;
      flags |= t[j].w >> 16;
    }
  }
  int tv, tt, tc, tl;
  int ev = block_excl_scan<1024>(sv, smem, &tv);
  int et = block_excl_scan<1024>(st, smem, &tt);
  int el = block_excl_scan<1024>(sl, smem, &tl);
  (void)block_excl_scan<1024>(sc, smem, &tc);
  const int has_neg = __syncthreads_or(flags & 1), has_pos = __syncthreads_or(flags & 2);
  for (int b = b0; b < b1; b += 8) {
    int4 t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = b + j < b1 ? run_tot[b + j] : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (b + j < b1) run_off[b + j] = make_int4(ev, et, 0, el);
      ev += t[j].x; et += t[j].y; el += t[j].w & 0xffff;
    }
  }
  if (threadIdx.x == 0) {
    const bool some = has_neg && has_pos && !no_cells;
    counts[0] = some ? tv : 0;
    counts[1] = some ? tt : 0;
    counts[2] = some ? tc : 0;
    counts[3] = (has_neg ? CNRMA_MESH_HAS_NEGATIVE : 0) | (has_pos ? CNRMA_MESH_HAS_POSITIVE : 0);
    header[0] = some ? tl : 0;
  }
}

struct MeshVolume {
  const float* tsdf;
  int X, Y, Z, YZ;
  __device__ __forceinline__ float g(size_t i) const { return mesh_field(tsdf[i]); }
  // gradient of g along one axis at voxel i (coordinate c of n, element stride s): central differences, one-sided at the border
  __device__ __forceinline__ float diff(size_t i, int c, int n, size_t s) const {
    if (n < 2) return 0.0f;
    if (c == 0) return g(i + s) - g(i);
    if (c == n - 1) return g(i) - g(i - s);
    return (g(i + s) - g(i - s)) * 0.5f;
  }
  __device__ __forceinline__ float3 grad(size_t i, int x, int y, int z) const {
    return make_float3(diff(i, x, X, (size_t)YZ), diff(i, y, Y, (size_t)Z), diff(i, z, Z, 1));
  }
};

// number of the vertex on the edge that leaves voxel o along `axis`
__device__ __forceinline__ int mesh_vertex_id(const MeshWave* __restrict__ waves, int o, int axis) {
  const uint4* p = reinterpret_cast<const uint4*>(waves + (o >> 6));
  const uint4 a = p[0], b = p[1];
  const unsigned long long bx = ((unsigned long long)a.y << 32) | a.x, by = ((unsigned long long)a.w << 32) | a.z;
  const unsigned long long bz = ((unsigned long long)b.y << 32) | b.x;
  const int l = o & 63;
  const unsigned long long below = (1ull << l) - 1ull;
  int id = (int)b.z + __popcll(bx & below) + __popcll(by & below) + __popcll(bz & below);
  if (axis > 0) id += (int)((bx >> l) & 1ull);
  if (axis > 1) id += (int)((by >> l) & 1ull);
  return id;
}

template <int AXIS>
__device__ __forceinline__ void mesh_emit_vertex(const MeshVolume& V, int k, int64_t v_cap, size_t i, int x, int y, int z, float g0,
                                                 float g1, float voxel_size, const float* __restrict__ origin,
                                                 float* __restrict__ vertices, float* __restrict__ normals) {
  if ((int64_t)k >= v_cap) return;
  const float t = g0 / (g0 - g1);
  float px = (float)x, py = (float)y, pz = (float)z;
  if (AXIS == 0) px += t;
  if (AXIS == 1) py += t;
  if (AXIS == 2) pz += t;
  float* v = vertices + (size_t)k * 3;
  v[0] = px * voxel_size + origin[0];
  v[1] = py * voxel_size + origin[1];
  v[2] = pz * voxel_size + origin[2];
  const float3 n0 = V.grad(i, x, y, z);
  const float3 n1 = V.grad(i + (AXIS == 0 ? (size_t)V.YZ : (AXIS == 1 ? (size_t)V.Z : 1)), x + (AXIS == 0), y + (AXIS == 1),
                           z + (AXIS == 2));
  const float nx = -(n0.x + t * (n1.x - n0.x)), ny = -(n0.y + t * (n1.y - n0.y)), nz = -(n0.z + t * (n1.z - n0.z));
  const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
  float* nn = normals + (size_t)k * 3;
  nn[0] = len > 0.0f ? nx / len : 0.0f;
  nn[1] = len > 0.0f ? ny / len : 0.0f;
  nn[2] = len > 0.0f ? nz / len : 0.0f;
}

__global__ __launch_bounds__(MESH_BLOCK) void mesh_emit_kernel(const float* __restrict__ tsdf, int X, int Y, int Z,
                                                               float voxel_size, const float* __restrict__ origin,
                                                               const int32_t* __restrict__ header,
                                                               const MeshWave* __restrict__ waves, const int2* __restrict__ list,
                                                               float* __restrict__ vertices, float* __restrict__ normals,
                                                               int64_t v_cap, int32_t* __restrict__ faces, int64_t f_cap,
                                                               const int32_t* __restrict__ counts) {
  const int n_list = header[0];
  v_cap = v_cap < counts[0] ? v_cap : counts[0];            // nothing is ever written behind the mesh's own end either
  f_cap = f_cap < counts[1] ? f_cap : counts[1];
  const MeshVolume V{tsdf, X, Y, Z, Y * Z};
  for (int e = blockIdx.x * MESH_BLOCK + threadIdx.x; e < n_list; e += gridDim.x * MESH_BLOCK) {
    const int2 rec = list[e];
    const int i = rec.x;
    const int x = i / V.YZ, r = i - x * V.YZ, y = r / Z, z = r - y * Z;
    const bool hx = x + 1 < X, hy = y + 1 < Y, hz = z + 1 < Z;
    const float g0 = V.g(i);
    const float gx = hx ? V.g((size_t)i + V.YZ) : 0.0f, gy = hy ? V.g((size_t)i + Z) : 0.0f, gz = hz ? V.g((size_t)i + 1) : 0.0f;
    const bool in0 = g0 > 0.0f;
    int k = mesh_vertex_id(waves, i, 0);
    if (hx && in0 != (gx > 0.0f)) mesh_emit_vertex<0>(V, k++, v_cap, i, x, y, z, g0, gx, voxel_size, origin, vertices, normals);
    if (hy && in0 != (gy > 0.0f)) mesh_emit_vertex<1>(V, k++, v_cap, i, x, y, z, g0, gy, voxel_size, origin, vertices, normals);
    if (hz && in0 != (gz > 0.0f)) mesh_emit_vertex<2>(V, k++, v_cap, i, x, y, z, g0, gz, voxel_size, origin, vertices, normals);
    if (!(hx && hy && hz)) continue;
    const size_t j = (size_t)i;
    const int cs = (int)in0 | ((int)(gx > 0.0f) << 1) | ((int)(gy > 0.0f) << 2) | ((int)(V.g(j + V.YZ + Z) > 0.0f) << 3) |
                   ((int)(gz > 0.0f) << 4) | ((int)(V.g(j + V.YZ + 1) > 0.0f) << 5) | ((int)(V.g(j + Z + 1) > 0.0f) << 6) |
                   ((int)(V.g(j + V.YZ + Z + 1) > 0.0f) << 7);
    const int nt = MESH_NTRI[cs];
    for (int t = 0; t < nt; ++t) {
      const int64_t f = (int64_t)rec.y + t;
      if (f >= f_cap) break;
      int id[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int edge = MESH_TRI[cs][3 * t + c], axis = edge >> 2, rank = edge & 3;
        const int corner = ((rank >> axis) << (axis + 1)) | (rank & ((1 << axis) - 1));      // the edge's start corner
        id[c] = mesh_vertex_id(waves, i + (corner & 1) * V.YZ + ((corner >> 1) & 1) * Z + (corner >> 2), axis);
      }
      int32_t* o = faces + (size_t)f * 3;
      o[0] = id[0];
      o[1] = id[1];
      o[2] = id[2];
    }
  }
}

}  // namespace

extern "C" size_t cnrma_mesh_workspace_bytes(int X, int Y, int Z) {
  if (!mesh_dims_ok(X, Y, Z)) return 0;
  return mesh_layout(X, Y, Z).total;
}

extern "C" int cnrma_mesh_count_f32(const float* tsdf, int X, int Y, int Z, void* workspace, size_t workspace_bytes,
                                    int32_t* counts, void* stream) {
  if (tsdf == nullptr || workspace == nullptr || counts == nullptr || !mesh_dims_ok(X, Y, Z)) return CNRMA_EINVAL;
  const MeshLayout L = mesh_layout(X, Y, Z);
  if (workspace_bytes < L.total || ((uintptr_t)workspace & 15) != 0) return CNRMA_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int4* run_tot = reinterpret_cast<int4*>(ws + L.run_tot);
  int4* run_off = reinterpret_cast<int4*>(ws + L.run_off);
  MeshWave* waves = reinterpret_cast<MeshWave*>(ws + L.waves);
  int2* list = reinterpret_cast<int2*>(ws + L.list);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)ceil_div(L.n_runs, MESH_BLOCK / 64)), block(MESH_BLOCK);
  if (Z < 64) hipLaunchKernelGGL(mesh_classify_kernel<true>, grid, block, 0, st, tsdf, Y, Z, (int)L.n, run_tot, waves);
  else hipLaunchKernelGGL(mesh_classify_kernel<false>, grid, block, 0, st, tsdf, Y, Z, (int)L.n, run_tot, waves);
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(1024), 0, st, run_tot, run_off, (int)L.n_runs,
                     (int)(X < 2 || Y < 2 || Z < 2), counts, reinterpret_cast<int32_t*>(ws + L.header));
  hipLaunchKernelGGL(mesh_compact_kernel, grid, block, 0, st, (int)L.n, run_off, waves, list);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_mesh_emit_f32(const float* tsdf, int X, int Y, int Z, float voxel_size, const float* origin3_dev,
                                   const void* workspace, float* vertices, float* normals, int64_t v_cap, int32_t* faces,
                                   int64_t f_cap, const int32_t* counts, void* stream) {
  if (tsdf == nullptr || workspace == nullptr || origin3_dev == nullptr || counts == nullptr || !mesh_dims_ok(X, Y, Z) ||
      v_cap < 0 || f_cap < 0 || (v_cap > 0 && (vertices == nullptr || normals == nullptr)) || (f_cap > 0 && faces == nullptr) ||
      ((uintptr_t)workspace & 15) != 0)
    return CNRMA_EINVAL;
  const MeshLayout L = mesh_layout(X, Y, Z);
  const char* ws = static_cast<const char*>(workspace);
  // a list entry writes at least one vertex or one triangle, so capacities that hold the mesh bound the list as well; a smaller
  // grid only strides further
  int64_t work = v_cap + f_cap < L.n ? v_cap + f_cap : L.n;
  int64_t blocks = ceil_div(work, MESH_BLOCK);
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  hipLaunchKernelGGL(mesh_emit_kernel, dim3((unsigned)blocks), dim3(MESH_BLOCK), 0, as_stream(stream), tsdf, X, Y, Z, voxel_size,
                     origin3_dev, reinterpret_cast<const int32_t*>(ws + L.header), reinterpret_cast<const MeshWave*>(ws + L.waves),
                     reinterpret_cast<const int2*>(ws + L.list), vertices, normals, v_cap, faces, f_cap, counts);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
