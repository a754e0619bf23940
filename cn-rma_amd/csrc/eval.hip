// Indoor mAP on the device (include/cnrma_eval.h): mmdet3d's indoor_eval as cnrma_amd.postprocess.indoor_eval restates it, for all
// scenes, classes and thresholds at once.  The host evaluator walks the detections of one (threshold, class, scene) at a time; the
// walk is not sequential by nature:
//   * a detection's best ground-truth box depends on its own scene and class alone                          (eval_best_kernel)
//   * it is a true positive at threshold t iff its best IoU exceeds t and it is the FIRST detection in score order among those
//     that chose the same box and exceed t: an unsigned minimum over sorted positions            (eval_claim_kernel, eval_flag_kernel)
//   * with the flags, AP is a scan over the class's stretch of the sorted list                                (eval_ap_kernel)
// Scenes arrive one at a time through eval_append_kernel: one workgroup, device-side cursors, nothing read back (capturable).
// The IoU is box_geom.h's, shared with nms.hip: every overlap rounds as cnrma_box_iou_f32's does.
#include <math.h>

#include "../../include/cnrma_eval.h"
#include "common.h"
#include "box_geom.h"

namespace {

constexpr int EVAL_MAX_T = 8;
constexpr int EVAL_BLOCK = 256;

__device__ __forceinline__ int32_t eval_label(const void* labels, int bytes, int64_t i) {
  if (bytes == 4) return static_cast<const int32_t*>(labels)[i];
  const int64_t v = static_cast<const int64_t*>(labels)[i];
  return (v < INT32_MIN || v > INT32_MAX) ? -1 : (int32_t)v;          // no class has such a label: the row matches nothing
}

__device__ __forceinline__ int32_t eval_clamp_i32(int64_t v, int64_t hi) { return (int32_t)(v < hi ? v : hi); }

struct EvalAppend {
  const float *boxes, *scores, *gt_boxes;
  const void *labels, *gt_labels;
  const int32_t* n_live;
  int box_cols, label_bytes, n_rows, gt_cols, gt_label_bytes, n_gt;
  float *det_boxes, *det_scores, *st_gt_boxes;
  int32_t *det_labels, *det_scene, *st_gt_labels, *scene_gt, *counters;
  int det_cap, gt_cap, scene_cap;
};

// APPEND: one workgroup.  Every thread reads the cursors, then the barrier, then the copies; thread 0 moves the cursors last, so no
// thread can see a moved cursor.  A destination row is written only below its capacity; the totals count every live row.
__global__ __launch_bounds__(1024) void eval_append_kernel(EvalAppend a) {
  const int tid = threadIdx.x;
  const int64_t d0 = a.counters[0], g0 = a.counters[1], s = a.counters[2];
  int n = a.n_rows;
  if (a.n_live != nullptr) n = min(a.n_rows, max(a.n_live[0], 0));
  __syncthreads();
  const bool writable = d0 >= 0 && g0 >= 0 && s >= 0 && s < a.scene_cap;
  if (writable) {
    const int64_t nd = min((int64_t)n, max((int64_t)a.det_cap - d0, (int64_t)0));        // rows that fit
    for (int64_t e = tid; e < nd * 7; e += 1024) {
      const int64_t r = e / 7;
      const int k = (int)(e - r * 7);
      a.det_boxes[(d0 + r) * 7 + k] = k < a.box_cols ? a.boxes[r * a.box_cols + k] : 0.0f;
    }
    for (int64_t r = tid; r < nd; r += 1024) {
      a.det_scores[d0 + r] = a.scores[r];
      a.det_labels[d0 + r] = eval_label(a.labels, a.label_bytes, r);
      a.det_scene[d0 + r] = (int32_t)s;
    }
    const int64_t ng = min((int64_t)a.n_gt, max((int64_t)a.gt_cap - g0, (int64_t)0));
    for (int64_t e = tid; e < ng * 7; e += 1024) {
      const int64_t r = e / 7;
      const int k = (int)(e - r * 7);
      a.st_gt_boxes[(g0 + r) * 7 + k] = k < a.gt_cols ? a.gt_boxes[r * a.gt_cols + k] : 0.0f;
    }
    for (int64_t r = tid; r < ng; r += 1024) a.st_gt_labels[g0 + r] = eval_label(a.gt_labels, a.gt_label_bytes, r);
  }
  if (tid == 0) {
    if (writable) {
      a.scene_gt[2 * s] = eval_clamp_i32(g0, a.gt_cap);
      a.scene_gt[2 * s + 1] = eval_clamp_i32(g0 + a.n_gt, a.gt_cap);
    }
    a.counters[0] = eval_clamp_i32(d0 + n, INT32_MAX);
    a.counters[1] = eval_clamp_i32(g0 + a.n_gt, INT32_MAX);
    a.counters[2] = eval_clamp_i32(s + 1, INT32_MAX);
  }
}

// BEST: one lane per detection; the lane looks up its own scene's ground-truth rows (a tile of lanes may span scenes), scans the
// boxes with its label in row order and keeps the first maximum (np.argmax).  IoUs are >= 0, so -1 is below every candidate.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_best_kernel(const float* __restrict__ det_boxes,
                                                               const int32_t* __restrict__ det_labels,
                                                               const int32_t* __restrict__ det_scene, int n_det,
                                                               const float* __restrict__ gt_boxes,
                                                               const int32_t* __restrict__ gt_labels, int n_gt,
                                                               const int32_t* __restrict__ scene_gt, int n_scenes, int rotated,
                                                               float* __restrict__ best_iou, int32_t* __restrict__ best_gt) {
  const int64_t i = (int64_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (i >= n_det) return;
  const int s = det_scene[i], label = det_labels[i];
  int g0 = 0, g1 = 0;
  if (s >= 0 && s < n_scenes) {
    g0 = min(max(scene_gt[2 * s], 0), n_gt);
    g1 = min(max(scene_gt[2 * s + 1], g0), n_gt);
  }
  const float* p = det_boxes + i * 7;
  float best = -1.0f;
  int bj = -1;
  for (int j = g0; j < g1; ++j) {
    if (gt_labels[j] != label) continue;
    const float v = box_iou3d(p, gt_boxes + (int64_t)j * 7, rotated);
    if (v > best) { best = v; bj = j; }
  }
  best_iou[i] = bj >= 0 ? best : 0.0f;
  best_gt[i] = bj;
}

struct EvalThresholds { float t[EVAL_MAX_T]; };

__device__ __forceinline__ EvalThresholds eval_thresholds(const float* __restrict__ thresholds, int T) {
  EvalThresholds th;
#pragma unroll
  for (int t = 0; t < EVAL_MAX_T; ++t) th.t[t] = t < T ? thresholds[t] : 2.0f;        // an IoU never exceeds 2
  return th;
}

// CLAIM: sorted position p -> claim[t][best_gt] = min(.., p) for every threshold the detection's best IoU exceeds
__global__ __launch_bounds__(EVAL_BLOCK) void eval_claim_kernel(const int64_t* __restrict__ order, int n_det,
                                                                const float* __restrict__ best_iou,
                                                                const int32_t* __restrict__ best_gt, int n_gt,
                                                                const float* __restrict__ thresholds, int T,
                                                                uint32_t* __restrict__ claim) {
  const int64_t p = (int64_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (p >= n_det) return;
  const int64_t i = order[p];
  if (i < 0 || i >= n_det) return;
  const int g = best_gt[i];
  if (g < 0 || g >= n_gt) return;
  const float v = best_iou[i];
  const EvalThresholds th = eval_thresholds(thresholds, T);
#pragma unroll
  for (int t = 0; t < EVAL_MAX_T; ++t)
    if (t < T && v > th.t[t]) atomicMin(&claim[(int64_t)t * n_gt + g], (uint32_t)p);
}

// FLAG: bit t = the detection holds the claim of its box at threshold t.  Written in row order (the caller's view) and in sorted
// order (what the AP scan streams).
__global__ __launch_bounds__(EVAL_BLOCK) void eval_flag_kernel(const int64_t* __restrict__ order, int n_det,
                                                               const float* __restrict__ best_iou,
                                                               const int32_t* __restrict__ best_gt, int n_gt,
                                                               const float* __restrict__ thresholds, int T,
                                                               const uint32_t* __restrict__ claim, uint8_t* __restrict__ flags,
                                                               uint8_t* __restrict__ flags_sorted) {
  const int64_t p = (int64_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
  if (p >= n_det) return;
  const int64_t i = order[p];
  uint32_t bits = 0;
  if (i >= 0 && i < n_det) {
    const int g = best_gt[i];
    if (g >= 0 && g < n_gt) {
      const float v = best_iou[i];
      const EvalThresholds th = eval_thresholds(thresholds, T);
#pragma unroll
      for (int t = 0; t < EVAL_MAX_T; ++t)
        if (t < T && v > th.t[t] && claim[(int64_t)t * n_gt + g] == (uint32_t)p) bits |= 1u << t;
    }
    flags[i] = (uint8_t)bits;
  }
  flags_sorted[p] = (uint8_t)bits;
}

// ---- block-wide helpers of the AP kernel (EVAL_BLOCK threads = 4 waves) ---------------------------------------------------------
constexpr int EVAL_WAVES = EVAL_BLOCK / 64;

__device__ __forceinline__ int eval_block_sum(int v, int* smem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v);
  if (lane == 63) smem[wid] = incl;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < EVAL_WAVES; ++w) total += smem[w];
  __syncthreads();
  return total;
}

__device__ __forceinline__ double eval_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// max over this lane and the lanes above it
__device__ __forceinline__ double eval_wave_suffix_max(double v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_down(v, d, 64);
    if (lane + d < 64) v = fmax(v, t);
  }
  return v;
}

// sorted position of the first detection whose label is >= c
__device__ __forceinline__ int eval_lower_bound(const int64_t* __restrict__ order, const int32_t* __restrict__ det_labels, int n_det,
                                                int64_t c) {
  int lo = 0, hi = n_det;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const int64_t i = order[mid];
    const int64_t l = (i >= 0 && i < n_det) ? (int64_t)det_labels[i] : (int64_t)INT32_MAX + 1;
    if (l < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// AP: one workgroup per (class, threshold).  The class's detections are the stretch [lo, hi) of the sorted list.  The envelope is a
// maximum over everything BEHIND a position, so the stretch is walked from its end in chunks of EVAL_BLOCK: the count of true
// positives in front of a chunk is the stretch's total (one pass ahead) minus what the chunks behind it and the chunk itself hold.
// The float64 sum runs in a fixed order (thread, then lanes, then waves): the result does not vary between runs.
__global__ __launch_bounds__(EVAL_BLOCK) void eval_ap_kernel(const int64_t* __restrict__ order,
                                                             const int32_t* __restrict__ det_labels, int n_det,
                                                             const int32_t* __restrict__ gt_labels, int n_gt,
                                                             const uint8_t* __restrict__ flags_sorted, int n_classes,
                                                             double* __restrict__ table) {
  __shared__ int s_cnt[EVAL_WAVES];
  __shared__ double s_max[EVAL_WAVES];
  __shared__ double s_sum[EVAL_WAVES];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int cnt = 0;
  for (int j = tid; j < n_gt; j += EVAL_BLOCK) cnt += gt_labels[j] == c;
  const int ngt = eval_block_sum(cnt, s_cnt);
  const int lo = eval_lower_bound(order, det_labels, n_det, c), hi = eval_lower_bound(order, det_labels, n_det, (int64_t)c + 1);
  const int m = hi - lo;
  const uint8_t* f = flags_sorted + lo;
  cnt = 0;
  for (int k = tid; k < m; k += EVAL_BLOCK) cnt += (f[k] >> t) & 1;
  const int total = eval_block_sum(cnt, s_cnt);
  const double dgt = (double)ngt;
  double env_behind = 0.0, acc = 0.0;           // mpre's closing 0: precisions are >= 0
  int run_end = total;                          // true positives up to the end of the current chunk
  for (int ch = (m + EVAL_BLOCK - 1) / EVAL_BLOCK - 1; ch >= 0; --ch) {
    const int k = ch * EVAL_BLOCK + tid;
    const bool live = k < m;
    const int tp = live ? (f[k] >> t) & 1 : 0;
    const int incl = wave_incl_scan(tp);
    if (lane == 63) s_cnt[wid] = incl;
    __syncthreads();
    int before = 0, chunk_total = 0;
#pragma unroll
    for (int w = 0; w < EVAL_WAVES; ++w) {
      const int v = s_cnt[w];
      if (w < wid) before += v;
      chunk_total += v;
    }
    const int ctp = run_end - chunk_total + before + incl;
    const double prec = live ? (double)ctp / fmax((double)(k + 1), 1e-9) : 0.0;
    const double wave_suf = eval_wave_suffix_max(prec);
    if (lane == 0) s_max[wid] = wave_suf;
    __syncthreads();
    double env = fmax(wave_suf, env_behind), chunk_max = 0.0;
#pragma unroll
    for (int w = 0; w < EVAL_WAVES; ++w) {
      const double v = s_max[w];
      if (w > wid) env = fmax(env, v);
      chunk_max = fmax(chunk_max, v);
    }
    if (tp && ngt > 0) acc += ((double)ctp / dgt - (double)(ctp - 1) / dgt) * env;
    env_behind = fmax(env_behind, chunk_max);
    run_end -= chunk_total;
  }
  const double wave_acc = eval_wave_sum(acc);
  if (lane == 0) s_sum[wid] = wave_acc;
  __syncthreads();
  if (tid == 0) {
    double ap = 0.0;
    for (int w = 0; w < EVAL_WAVES; ++w) ap += s_sum[w];
    double* row = table + ((int64_t)t * n_classes + c) * 4;
    row[0] = ngt > 0 ? ap : 0.0;
    row[1] = ngt > 0 ? (double)total / dgt : 0.0;
    row[2] = dgt;
    row[3] = (double)m;
  }
}

static inline size_t eval_align16(size_t b) { return (b + 15) & ~(size_t)15; }

struct EvalWorkspace {
  uint32_t* claim;           // [T][n_gt]
  uint8_t* flags_sorted;     // [n_det]
};

static inline size_t eval_workspace_layout(int n_det, int n_gt, int T, void* base, EvalWorkspace* ws) {
  const size_t claim_b = eval_align16((size_t)T * (size_t)n_gt * sizeof(uint32_t));
  const size_t flags_b = eval_align16((size_t)n_det);
  if (ws != nullptr) {
    char* p = static_cast<char*>(base);
    ws->claim = reinterpret_cast<uint32_t*>(p);
    ws->flags_sorted = reinterpret_cast<uint8_t*>(p + claim_b);
  }
  return claim_b + flags_b + 16;            // never 0 for valid arguments: 0 is the query's "refused"
}

}  // namespace

extern "C" int cnrma_eval_abi_version(void) { return CNRMA_EVAL_ABI_VERSION; }

extern "C" int cnrma_eval_reset(int32_t* counters, void* stream) {
  if (counters == nullptr) return CNRMA_EVAL_EINVAL;
  const hipError_t e = cnrma_fill_bytes(counters, 0, 4 * sizeof(int32_t), as_stream(stream));
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int cnrma_eval_append_f32(const float* boxes, int box_cols, const float* scores, const void* labels, int label_bytes,
                                     int n_rows, const int32_t* n_live, const float* gt_boxes, int gt_cols, const void* gt_labels,
                                     int gt_label_bytes, int n_gt, float* st_det_boxes, float* st_det_scores,
                                     int32_t* st_det_labels, int32_t* st_det_scene, int det_cap, float* st_gt_boxes,
                                     int32_t* st_gt_labels, int gt_cap, int32_t* st_scene_gt, int scene_cap, int32_t* counters,
                                     void* stream) {
  if (n_rows < 0 || n_gt < 0 || det_cap < 0 || gt_cap < 0 || scene_cap < 0 || (box_cols != 6 && box_cols != 7) ||
      (gt_cols != 6 && gt_cols != 7) || (label_bytes != 4 && label_bytes != 8) || (gt_label_bytes != 4 && gt_label_bytes != 8) ||
      counters == nullptr)
    return CNRMA_EVAL_EINVAL;
  if (n_rows > 0 && (boxes == nullptr || scores == nullptr || labels == nullptr)) return CNRMA_EVAL_EINVAL;
  if (n_gt > 0 && (gt_boxes == nullptr || gt_labels == nullptr)) return CNRMA_EVAL_EINVAL;
  if (det_cap > 0 && (st_det_boxes == nullptr || st_det_scores == nullptr || st_det_labels == nullptr || st_det_scene == nullptr))
    return CNRMA_EVAL_EINVAL;
  if (gt_cap > 0 && (st_gt_boxes == nullptr || st_gt_labels == nullptr)) return CNRMA_EVAL_EINVAL;
  if (scene_cap > 0 && st_scene_gt == nullptr) return CNRMA_EVAL_EINVAL;
  EvalAppend a;
  a.boxes = boxes; a.scores = scores; a.gt_boxes = gt_boxes;
  a.labels = labels; a.gt_labels = gt_labels;
  a.n_live = n_live;
  a.box_cols = box_cols; a.label_bytes = label_bytes; a.n_rows = n_rows;
  a.gt_cols = gt_cols; a.gt_label_bytes = gt_label_bytes; a.n_gt = n_gt;
  a.det_boxes = st_det_boxes; a.det_scores = st_det_scores; a.st_gt_boxes = st_gt_boxes;
  a.det_labels = st_det_labels; a.det_scene = st_det_scene; a.st_gt_labels = st_gt_labels;
  a.scene_gt = st_scene_gt; a.counters = counters;
  a.det_cap = det_cap; a.gt_cap = gt_cap; a.scene_cap = scene_cap;
  hipLaunchKernelGGL(eval_append_kernel, dim3(1), dim3(1024), 0, as_stream(stream), a);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cnrma_eval_result_workspace_bytes(int n_det, int n_gt, int T) {
  if (n_det < 0 || n_gt < 0 || T < 1 || T > EVAL_MAX_T) return 0;
  return eval_workspace_layout(n_det, n_gt, T, nullptr, nullptr);
}

extern "C" int cnrma_eval_result_f32(const float* det_boxes, const int32_t* det_labels, const int32_t* det_scene, int n_det,
                                     const float* gt_boxes, const int32_t* gt_labels, int n_gt, const int32_t* scene_gt,
                                     int n_scenes, int rotated, const int64_t* order, const float* thresholds, int T,
                                     int n_classes, void* workspace, size_t workspace_bytes, float* best_iou, int32_t* best_gt,
                                     uint8_t* flags, double* table, void* stream) {
  if (n_det < 0 || n_gt < 0 || n_scenes < 0 || T < 1 || T > EVAL_MAX_T || n_classes < 1 || thresholds == nullptr || table == nullptr || workspace == nullptr || ((uintptr_t)workspace & 15) != 0)
    return CNRMA_EVAL_EINVAL;
  if (n_det > 0 && (det_boxes == nullptr || det_labels == nullptr || det_scene == nullptr || order == nullptr ||
                    best_iou == nullptr || best_gt == nullptr || flags == nullptr || (n_scenes > 0 && scene_gt == nullptr)))
    return CNRMA_EVAL_EINVAL;
  if (n_gt > 0 && (gt_boxes == nullptr || gt_labels == nullptr)) return CNRMA_EVAL_EINVAL;
  EvalWorkspace ws;
  if (workspace_bytes < eval_workspace_layout(n_det, n_gt, T, workspace, &ws)) return CNRMA_EVAL_EINVAL;
  hipStream_t st = as_stream(stream);
  if (n_det > 0) {
    const unsigned blocks = (unsigned)ceil_div(n_det, EVAL_BLOCK);
    hipLaunchKernelGGL(eval_best_kernel, dim3(blocks), dim3(EVAL_BLOCK), 0, st, det_boxes, det_labels, det_scene, n_det, gt_boxes,
                       gt_labels, n_gt, scene_gt, n_scenes, rotated, best_iou, best_gt);
    CNRMA_LAUNCH_CHECK();
    if (n_gt > 0) {
      const hipError_t e = cnrma_fill_bytes(ws.claim, 0xFF, (size_t)T * n_gt * sizeof(uint32_t), st);
      if (e != hipSuccess) return -(int)e;
      hipLaunchKernelGGL(eval_claim_kernel, dim3(blocks), dim3(EVAL_BLOCK), 0, st, order, n_det, best_iou, best_gt, n_gt,
                         thresholds, T, ws.claim);
      CNRMA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(eval_flag_kernel, dim3(blocks), dim3(EVAL_BLOCK), 0, st, order, n_det, best_iou, best_gt, n_gt, thresholds,
                       T, ws.claim, flags, ws.flags_sorted);
    CNRMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(eval_ap_kernel, dim3(n_classes, T), dim3(EVAL_BLOCK), 0, st, order, det_labels, n_det, gt_labels, n_gt,
                     ws.flags_sorted, n_classes, table);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
