// 3D NMS for the offline post-processing step: BEV-overlap NMS as used by the reference's
// post_process/nms_bbox.py:17-58 through mmdet3d's pcdet_nms_gpu (rotated boxes) / pcdet_nms_normal_gpu (axis-aligned).
// Third-party semantics (OpenPCDet iou3d_nms, not under /root/reference): boxes are (x, y, z, dx, dy, dz, heading),
// the overlap is the 2D IoU of the bird's-eye-view rectangles, candidates are visited in descending score order and a
// candidate is dropped when its IoU with an already kept box exceeds the threshold.
//
// Kernel: one 64 x 64 tile of the pairwise suppression matrix per block -> bit mask [N][ceil(N/64)] (uint64);
// the greedy pass over the mask is a sequential scan done by the host wrapper (post-processing, not the hot path).
//
// cnrma_nms_classes_f32 is the same NMS for ALL classes of a scene in four launches and without a host in the loop
// (rank -> mask -> scan -> gather, below): it takes the padded detection block of the static trace and is capturable.
#include "common.h"
#include "box_geom.h"      // P2, bev_corners, quad_intersection_area, rotated_bev_intersection (shared with eval.hip)

namespace {

__device__ __forceinline__ float bev_iou(const float* a, const float* b, int rotated) {
  float inter;
  if (rotated) {
    inter = rotated_bev_intersection(a, b);
  } else {
    const float lx = fmaxf(a[0] - a[3] * 0.5f, b[0] - b[3] * 0.5f), rx = fminf(a[0] + a[3] * 0.5f, b[0] + b[3] * 0.5f);
    const float ly = fmaxf(a[1] - a[4] * 0.5f, b[1] - b[4] * 0.5f), ry = fminf(a[1] + a[4] * 0.5f, b[1] + b[4] * 0.5f);
    inter = fmaxf(rx - lx, 0.0f) * fmaxf(ry - ly, 0.0f);
  }
  const float uni = a[3] * a[4] + b[3] * b[4] - inter;
  return inter / fmaxf(uni, 1e-8f);
}

// boxes [N][7] sorted by descending score; mask[i][j/64] bit (j%64) set when j > i and IoU(i, j) > thr
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, int n, float thr, int rotated,
                                                      unsigned long long* __restrict__ mask, int words) {
  const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
  if (col0 + 63 < row0) return;                      // strictly below the diagonal: never needed
  __shared__ float cb[64 * 7];
  const int tid = threadIdx.x;
  if (col0 + tid < n)
    for (int k = 0; k < 7; ++k) cb[tid * 7 + k] = boxes[(int64_t)(col0 + tid) * 7 + k];
  __syncthreads();
  const int i = row0 + tid;
  if (i >= n) return;
  float a[7];
  for (int k = 0; k < 7; ++k) a[k] = boxes[(int64_t)i * 7 + k];
  unsigned long long bits = 0ull;
  const int lim = min(64, n - col0);
  for (int j = 0; j < lim; ++j) {
    if (col0 + j <= i) continue;
    if (bev_iou(a, cb + j * 7, rotated) > thr) bits |= 1ull << j;
  }
  mask[(int64_t)i * words + blockIdx.x] = bits;
}

// pairwise IoU matrix (evaluation / tests): iou[i][j] for a [Na][7], b [Nb][7]; mode 0 = BEV, 1 = 3D (BEV x height)
__global__ __launch_bounds__(256) void iou_matrix_kernel(const float* __restrict__ a, int na, const float* __restrict__ b,
                                                         int nb, int rotated, int mode3d, float* __restrict__ iou) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)na * nb) return;
  const int i = (int)(t / nb), j = (int)(t - (int64_t)i * nb);
  const float* p = a + (int64_t)i * 7;
  const float* q = b + (int64_t)j * 7;
  if (!mode3d) { iou[t] = bev_iou(p, q, rotated); return; }
  float inter;
  if (rotated) {
    inter = rotated_bev_intersection(p, q);
  } else {
    const float lx = fmaxf(p[0] - p[3] * 0.5f, q[0] - q[3] * 0.5f), rx = fminf(p[0] + p[3] * 0.5f, q[0] + q[3] * 0.5f);
    const float ly = fmaxf(p[1] - p[4] * 0.5f, q[1] - q[4] * 0.5f), ry = fminf(p[1] + p[4] * 0.5f, q[1] + q[4] * 0.5f);
    inter = fmaxf(rx - lx, 0.0f) * fmaxf(ry - ly, 0.0f);
  }
  const float zl = fmaxf(p[2] - p[5] * 0.5f, q[2] - q[5] * 0.5f), zh = fminf(p[2] + p[5] * 0.5f, q[2] + q[5] * 0.5f);
  const float iv = inter * fmaxf(zh - zl, 0.0f);
  const float uv = p[3] * p[4] * p[5] + q[3] * q[4] * q[5] - iv;
  iou[t] = iv / fmaxf(uv, 1e-8f);
}

// ---- all classes of a scene on the device ------------------------------------------------------------------------------------
// Workspace of one call (n_cap rows, W = ceil(n_cap / 64) words per mask row), per class c:
//   mask  uint64 [n_cap][W]   suppression bits in RANK order, written only where the scan reads (see nms_classes_mask_kernel)
//   order int32  [n_cap]      padded row of rank k (descending score, ties by lower row)
//   kept  int32  [n_cap]      padded rows of the kept boxes, in rank order
// and two int32 [n_cls] vectors: n_c (candidates) and n_keep (kept boxes).
constexpr int NMS_MAX_ROWS = 4096;         // 64 lanes x 64 bits: one wave holds a class's whole `removed` set in registers
constexpr int NMS_MAX_SEGMENTS = 8;

struct NmsSegments { int n, size[NMS_MAX_SEGMENTS]; };

struct NmsWorkspace {
  unsigned long long* mask;
  int32_t *order, *kept, *n_c, *n_keep;
};

static inline size_t nms_align16(size_t b) { return (b + 15) & ~(size_t)15; }

static inline size_t nms_workspace_layout(int n_cap, int n_cls, void* base, NmsWorkspace* ws) {
  const size_t words = (size_t)(n_cap + 63) / 64;
  const size_t mask_b = nms_align16((size_t)n_cls * n_cap * words * sizeof(uint64_t));
  const size_t rows_b = nms_align16((size_t)n_cls * n_cap * sizeof(int32_t));
  const size_t cls_b = nms_align16((size_t)n_cls * sizeof(int32_t));
  if (ws != nullptr) {
    char* p = static_cast<char*>(base);
    ws->mask = reinterpret_cast<unsigned long long*>(p);
    ws->order = reinterpret_cast<int32_t*>(p + mask_b);
    ws->kept = reinterpret_cast<int32_t*>(p + mask_b + rows_b);
    ws->n_c = reinterpret_cast<int32_t*>(p + mask_b + 2 * rows_b);
    ws->n_keep = reinterpret_cast<int32_t*>(p + mask_b + 2 * rows_b + cls_b);
  }
  return mask_b + 2 * rows_b + 2 * cls_b;
}

// RANK: one workgroup per class.  A live row with score > thr (NaN never passes) gets the key (descending score, row):
// the order-preserving transform of the float, inverted, in the high half and the padded row in the low half; every other row
// the all-ones sentinel.  A bitonic network sorts the P = 2^k >= n_cap keys in LDS; ascending keys = torch's stable descending
// sort of the class's candidates (equal scores, -0.0 and +0.0 among them, go by the lower row).
__global__ __launch_bounds__(1024) void nms_classes_rank_kernel(const float* __restrict__ scores, int n_cap, int n_cls,
                                                                 NmsSegments seg, const int32_t* __restrict__ valid,
                                                                 float score_thr, int P, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ n_c) {
  __shared__ unsigned long long key[NMS_MAX_ROWS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const unsigned long long SENT = ~0ull;
  for (int r = tid; r < P; r += 1024) {
    unsigned long long k = SENT;
    if (r < n_cap) {
      int r0 = 0;
      bool live = false;
      for (int l = 0; l < seg.n; ++l) {
        if (r >= r0 && r < r0 + seg.size[l]) {
          const int v = valid != nullptr ? min(valid[l], seg.size[l]) : seg.size[l];
          live = r - r0 < v;
        }
        r0 += seg.size[l];
      }
      if (live) {
        float s = scores[(int64_t)r * n_cls + c];
        if (s > score_thr) {
          if (s == 0.0f) s = 0.0f;                                  // -0.0 ties with +0.0, as in a float comparison
          const uint32_t u = __float_as_uint(s);
          const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
          k = ((unsigned long long)(~asc) << 32) | (uint32_t)r;
        }
      }
    }
    key[r] = k;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += 1024) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = key[lo], b = key[hi];
        if ((a > b) == up) { key[lo] = b; key[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < P; r += 1024) {
    const unsigned long long k = key[r];
    if (r < n_cap) order[(int64_t)c * n_cap + r] = k == SENT ? 0 : (int32_t)(uint32_t)k;
    if (k != SENT && (r + 1 == P || key[r + 1] == SENT)) n_c[c] = r + 1;      // the last candidate
    if (r == 0 && k == SENT) n_c[c] = 0;
  }
}

// MASK: nms_mask_kernel over a (W, W, n_cls) grid, the boxes gathered through `order` (six-wide boxes get yaw 0).  Tiles beyond
// the class's candidates or below the diagonal exit at once, so of row i < n_c exactly the words w with i / 64 <= w and
// 64 w < n_c are written -- the words the scan reads; nothing is cleared.
__global__ __launch_bounds__(64) void nms_classes_mask_kernel(const float* __restrict__ boxes, int cols, int n_cap,
                                                              const int32_t* __restrict__ order, const int32_t* __restrict__ n_c,
                                                              float thr, unsigned long long* __restrict__ mask, int words) {
  const int c = blockIdx.z, n = min(n_c[c], n_cap);
  const int row0 = blockIdx.y * 64, col0 = blockIdx.x * 64;
  if (row0 >= n || col0 >= n || col0 + 63 < row0) return;
  __shared__ float cb[64 * 7];
  const int tid = threadIdx.x;
  const int32_t* ord = order + (int64_t)c * n_cap;
  const int rotated = cols == 7;
  if (col0 + tid < n) {
    const float* src = boxes + (int64_t)ord[col0 + tid] * cols;
    for (int k = 0; k < 6; ++k) cb[tid * 7 + k] = src[k];
    cb[tid * 7 + 6] = rotated ? src[6] : 0.0f;
  }
  __syncthreads();
  const int i = row0 + tid;
  if (i >= n) return;
  float a[7];
  {
    const float* src = boxes + (int64_t)ord[i] * cols;
    for (int k = 0; k < 6; ++k) a[k] = src[k];
    a[6] = rotated ? src[6] : 0.0f;
  }
  unsigned long long bits = 0ull;
  const int lim = min(64, n - col0);
  for (int j = 0; j < lim; ++j) {
    if (col0 + j <= i) continue;
    if (bev_iou(a, cb + j * 7, rotated) > thr) bits |= 1ull << j;
  }
  mask[((int64_t)c * n_cap + i) * words + blockIdx.x] = bits;
}

__device__ __forceinline__ unsigned long long wave_read64(unsigned long long v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// SCAN: one wave per class; lane l holds the `removed` word of ranks 64 l .. 64 l + 63 in a register.  The ranks are walked in
// blocks of 64.  Whether rank 64 b + j survives depends, inside its block, only on the diagonal tile: its 64 words are fetched
// with one load (lane j = row j) and the block's greedy pass then runs on registers alone -- readlane of the diagonal word of each
// kept rank, a scalar branch per rank, no memory in the chain.  The mask rows of the block's kept ranks (512 bytes each, lane =
// word) do not depend on one another any more: they are requested four at a time and ORed into `removed`.  Kept ranks are
// compacted in rank order by popcount and a lane prefix.
__global__ __launch_bounds__(64) void nms_classes_scan_kernel(const unsigned long long* __restrict__ mask, int n_cap, int words,
                                                              const int32_t* __restrict__ order, const int32_t* __restrict__ n_c,
                                                              int32_t* __restrict__ kept, int32_t* __restrict__ n_keep) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(min(n_c[c], n_cap));
  const unsigned long long* m = mask + (int64_t)c * n_cap * words;
  const int32_t* ord = order + (int64_t)c * n_cap;
  int32_t* out = kept + (int64_t)c * n_cap;
  const bool word_live = lane < words && lane * 64 < n;           // this lane's word was written by every row above it
  unsigned long long removed = 0ull;
  int total = 0;
  for (int b = 0; b * 64 < n; ++b) {
    const int rank = b * 64 + lane;
    const unsigned long long diag = rank < n ? m[(int64_t)rank * words + b] : 0ull;
    const int in_block = min(64, n - b * 64);
    unsigned long long gone = wave_read64(removed, b);
    if (in_block < 64) gone |= ~0ull << in_block;                  // ranks behind the last candidate
    unsigned long long keep_bits = 0ull;
    while (~gone != 0ull) {
      const int j = __builtin_ctzll(~gone);
      keep_bits |= 1ull << j;
      gone |= wave_read64(diag, j) | (1ull << j);
    }
    // kept ranks of the block -> their rows, ORed into the words to the right of the diagonal
    const bool take = word_live && lane > b;
    unsigned long long rest = keep_bits;
    while (rest != 0ull) {
      int j[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        j[u] = rest != 0ull ? __builtin_ctzll(rest) : -1;
        rest &= rest - 1ull;
      }
      unsigned long long row[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) row[u] = (take && j[u] >= 0) ? m[(int64_t)(b * 64 + j[u]) * words + lane] : 0ull;
      removed |= (row[0] | row[1]) | (row[2] | row[3]);
    }
    if ((keep_bits >> lane) & 1ull) out[total + __builtin_popcountll(keep_bits & ((1ull << lane) - 1ull))] = ord[rank];
    total += __builtin_popcountll(keep_bits);
  }
  if (lane == 0) n_keep[c] = total;
}

// GATHER: class c's kept rows go behind those of the classes before it (exclusive scan of n_keep), in rank order: the order of
// postprocess.nms.  n_out[0] = the true total, rows from out_cap on are dropped.
__global__ __launch_bounds__(256) void nms_classes_gather_kernel(const float* __restrict__ boxes, int cols,
                                                                 const float* __restrict__ scores, int n_cap, int n_cls,
                                                                 const int32_t* __restrict__ kept, const int32_t* __restrict__ n_keep,
                                                                 float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                                 int64_t* __restrict__ out_labels, int out_cap,
                                                                 int32_t* __restrict__ n_out) {
  const int c = blockIdx.x;
  int off = 0, total = 0;
  for (int k = 0; k < n_cls; ++k) {
    const int v = n_keep[k];
    if (k < c) off += v;
    total += v;
  }
  if (c == 0 && threadIdx.x == 0) n_out[0] = total;
  const int n = n_keep[c];
  for (int k = threadIdx.x; k < n; k += 256) {
    const int o = off + k;
    if (o >= out_cap) break;
    const int r = kept[(int64_t)c * n_cap + k];
    for (int q = 0; q < cols; ++q) out_boxes[(int64_t)o * cols + q] = boxes[(int64_t)r * cols + q];
    out_scores[o] = scores[(int64_t)r * n_cls + c];
    out_labels[o] = c;
  }
}

}  // namespace

extern "C" int cnrma_nms_mask_f32(const float* boxes_sorted, int n, float iou_thr, int rotated, uint64_t* mask,
                                  void* stream) {
  if (n <= 0) return n == 0 ? 0 : CNRMA_EINVAL;
  const int words = (n + 63) / 64;
  hipStream_t st = as_stream(stream);
  hipError_t e = cnrma_fill_bytes(mask, 0, (size_t)n * words * sizeof(uint64_t), st);
  if (e != hipSuccess) return -(int)e;
  hipLaunchKernelGGL(nms_mask_kernel, dim3(words, words), dim3(64), 0, st, boxes_sorted, n, iou_thr, rotated,
                     reinterpret_cast<unsigned long long*>(mask), words);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" int cnrma_box_iou_f32(const float* a, int na, const float* b, int nb, int rotated, int mode3d, float* iou,
                                 void* stream) {
  if (na <= 0 || nb <= 0) return (na == 0 || nb == 0) ? 0 : CNRMA_EINVAL;
  hipLaunchKernelGGL(iou_matrix_kernel, dim3((unsigned)ceil_div((int64_t)na * nb, 256)), dim3(256), 0, as_stream(stream),
                     a, na, b, nb, rotated, mode3d, iou);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cnrma_nms_classes_workspace_bytes(int n_cap, int n_cls) {
  if (n_cap < 0 || n_cap > NMS_MAX_ROWS || n_cls <= 0) return 0;
  return nms_workspace_layout(n_cap, n_cls, nullptr, nullptr);
}

extern "C" int cnrma_nms_classes_f32(const float* boxes, int box_cols, const float* scores, int n_cap, int n_cls,
                                     const int32_t* sizes, int n_segments, const int32_t* valid, float score_thr,
                                     float iou_thr, void* workspace, size_t workspace_bytes, float* out_boxes,
                                     float* out_scores, int64_t* out_labels, int out_cap, int32_t* n_out, void* stream) {
  if (n_cap < 0 || n_cap > NMS_MAX_ROWS || n_cls <= 0 || n_cls > 65535 || (box_cols != 6 && box_cols != 7) || out_cap < 0 ||
      n_segments < 1 || n_segments > NMS_MAX_SEGMENTS || sizes == nullptr || n_out == nullptr)
    return CNRMA_EINVAL;
  NmsSegments seg;
  seg.n = n_segments;
  int64_t rows = 0;
  for (int l = 0; l < NMS_MAX_SEGMENTS; ++l) {
    seg.size[l] = l < n_segments ? sizes[l] : 0;
    if (seg.size[l] < 0) return CNRMA_EINVAL;
    rows += seg.size[l];
  }
  if (rows != n_cap) return CNRMA_EINVAL;
  hipStream_t st = as_stream(stream);
  if (n_cap == 0) {
    hipError_t e = cnrma_fill_bytes(n_out, 0, sizeof(int32_t), st);
    return e == hipSuccess ? 0 : -(int)e;
  }
  NmsWorkspace ws;
  if (workspace == nullptr || workspace_bytes < nms_workspace_layout(n_cap, n_cls, workspace, &ws)) return CNRMA_EINVAL;
  const int words = (n_cap + 63) / 64;
  int P = 2;
  while (P < n_cap) P <<= 1;
  hipLaunchKernelGGL(nms_classes_rank_kernel, dim3(n_cls), dim3(1024), 0, st, scores, n_cap, n_cls, seg, valid, score_thr, P,
                     ws.order, ws.n_c);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_classes_mask_kernel, dim3(words, words, n_cls), dim3(64), 0, st, boxes, box_cols, n_cap, ws.order,
                     ws.n_c, iou_thr, ws.mask, words);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_classes_scan_kernel, dim3(n_cls), dim3(64), 0, st, ws.mask, n_cap, words, ws.order, ws.n_c, ws.kept,
                     ws.n_keep);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(nms_classes_gather_kernel, dim3(n_cls), dim3(256), 0, st, boxes, box_cols, scores, n_cap, n_cls, ws.kept,
                     ws.n_keep, out_boxes, out_scores, out_labels, out_cap, n_out);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
