// FCAF3D training targets and detection losses on the device (include/cnrma.h "a13"):
//   cnrma_fcaf3d_assign_f32           FCAF3DAssigner.assign (fcaf3d_head.py:405-484) without any [n, m] plane
//   cnrma_fcaf3d_focal_loss_f32       sigmoid focal loss over [n_cap][n_cls] logits + its gradient, no one-hot tensor
//   cnrma_fcaf3d_positive_losses_f32  centerness BCE and IoU3D loss (axis-aligned or rotated about z) over the positive rows
// Every entry point is a linear chain of launches on one stream; no allocation, no synchronisation, no host read: all of it
// can be captured in a graph.  Counts are integer atomics, the k-th value is a radix select on the float bits and every
// floating-point sum is combined in one fixed order in fp64, so every output is the same replay to replay.
//
// Assignment (six launches): clear -> count (inside points per level and box) -> kth (best level + the k-th largest
// centerness of each box's column, one workgroup per box over the rows of its best level only) -> assign (per row: the
// smallest-volume box among those that pass the three conditions) -> scan (per-block positive counts -> offsets, n_pos, tail
// rows) -> compact (positive rows in ascending row order).
// The face distances are evaluated in the operation order of the torch code (-ffp-contract=off: no fused multiply-add), so
// `> 0`, the centerness bits and with them the k-th value and the strict comparison against it agree bit for bit with
// FCAF3DAssigner.assign run in fp32 on the CPU.
//
// The two loss kernels evaluate their element math in fp64 (the inputs and outputs are fp32): ~11 M logits x ~200 fp64
// operations is ~0.1 ms on this part, and the result then carries the rounding of one fp32 store instead of a chain of fp32
// exp / log1p / divisions.  The rotated IoU carries the seven partial derivatives of the decoded box through the polygon
// computation as forward-mode duals, per thread.
#include "common.h"

namespace {

constexpr int TGT_MAX_LEVELS = 8;
constexpr int TGT_MAX_BOXES = 1024;
constexpr int TGT_BLOCK = 256;
constexpr int TGT_KTH_BLOCK = 1024;
constexpr float TGT_BIG_VOLUME = 1e8f;        // `big` of FCAF3DAssigner.assign: a box at or above it never wins a row

// the levels of the concatenated row set: level l owns rows [start[l], start[l + 1]) and blocks [block0[l], block0[l + 1]) of the
// flat row grid (TGT_BLOCK rows per block; a block never straddles two levels)
struct TgtLevels {
  int n;
  int32_t start[TGT_MAX_LEVELS + 1];
  int32_t block0[TGT_MAX_LEVELS + 1];
};

__device__ __forceinline__ int tgt_level_of_block(const TgtLevels& lv, int b) {
  int l = 0;
  for (int i = 1; i < lv.n; ++i)
    if (b >= lv.block0[i]) l = i;
  return l;
}

__device__ __forceinline__ int tgt_level_live(const TgtLevels& lv, const int32_t* level_live, int l) {
  const int cap = lv.start[l + 1] - lv.start[l];
  if (level_live == nullptr) return cap;
  const int v = level_live[l];
  return v < 0 ? 0 : (v < cap ? v : cap);
}

__device__ __forceinline__ int tgt_box_count(const int32_t* m_live, int m_cap) {
  const int v = m_live[0];
  return v < 0 ? 0 : (v < m_cap ? v : m_cap);
}

// the six face distances of a point to box j (fcaf3d_head.py:504-514), in the order (x lo, x hi, y lo, y hi, z lo, z hi);
// true when the point lies strictly inside (condition 1)
__device__ __forceinline__ bool tgt_faces(float px, float py, float pz, const float* __restrict__ b, const float* __restrict__ cs,
                                          float* t) {
  const float c0 = b[0], c1 = b[1], c2 = b[2];
  const float r0 = px - c0, r1 = py - c1, r2 = pz - c2;
  const float c = cs[0], s = cs[1];
  const float q0 = r0 * c + r1 * s;
  const float q1 = (-r0) * s + r1 * c;
  const float x = c0 + q0, y = c1 + q1, z = c2 + r2;
  const float hx = b[3] / 2, hy = b[4] / 2, hz = b[5] / 2;
  t[0] = (x - c0) + hx; t[1] = (c0 + hx) - x;
  t[2] = (y - c1) + hy; t[3] = (c1 + hy) - y;
  t[4] = (z - c2) + hz; t[5] = (c2 + hz) - z;
  return t[0] > 0.f && t[1] > 0.f && t[2] > 0.f && t[3] > 0.f && t[4] > 0.f && t[5] > 0.f;
}

// compute_centerness (fcaf3d_head.py:395-402): ((((xmin / xmax) * ymin) / ymax) * zmin) / zmax, then the square root
__device__ __forceinline__ float tgt_centerness(const float* t) {
  float c = fminf(t[0], t[1]) / fmaxf(t[0], t[1]);
  c = c * fminf(t[2], t[3]);
  c = c / fmaxf(t[2], t[3]);
  c = c * fminf(t[4], t[5]);
  c = c / fmaxf(t[4], t[5]);
  return sqrtf(c);
}

// ---- count: inside points per (level, box) ------------------------------------------------------------------------------
__global__ __launch_bounds__(TGT_BLOCK) void tgt_count_kernel(const float* __restrict__ points, TgtLevels lv,
                                                              const int32_t* __restrict__ level_live,
                                                              const float* __restrict__ boxes, const float* __restrict__ cs,
                                                              int m_cap, const int32_t* __restrict__ m_live,
                                                              int32_t* __restrict__ counts) {
  extern __shared__ int32_t s_cnt[];                     // [m_cap]
  const int m = tgt_box_count(m_live, m_cap);
  const int l = tgt_level_of_block(lv, blockIdx.x);
  const int first = lv.start[l] + ((int)blockIdx.x - lv.block0[l]) * TGT_BLOCK;
  const int live_end = lv.start[l] + tgt_level_live(lv, level_live, l);
  if (first >= live_end || m == 0) return;                // uniform over the block
  for (int j = threadIdx.x; j < m; j += TGT_BLOCK) s_cnt[j] = 0;
  __syncthreads();
  const int row = first + threadIdx.x;
  const bool alive = row < live_end;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (alive) { px = points[3 * (int64_t)row]; py = points[3 * (int64_t)row + 1]; pz = points[3 * (int64_t)row + 2]; }
  for (int j = 0; j < m; ++j) {
    float t[6];
    const bool in = tgt_faces(px, py, pz, boxes + 7 * j, cs + 2 * j, t) && alive;
    const unsigned long long bal = __ballot(in);
    if (bal != 0ull && (threadIdx.x & 63) == 0) atomicAdd(&s_cnt[j], __popcll(bal));
  }
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += TGT_BLOCK)
    if (s_cnt[j] != 0) atomicAdd(&counts[l * m_cap + j], s_cnt[j]);
}

// ---- kth: best level of a box and the k-th largest centerness of its column (k = min(topk + 1, n)) ----------------------------
// One workgroup per box.  Non-candidates count as -1 in the column, candidates are >= 0: with fewer than k candidates the k-th
// value is -1, otherwise it is the k-th largest candidate, found by a four-pass radix select on the float bits (a value >= 0
// orders like its bit pattern) over the live rows of the best level -- the only rows that can be candidates.
__global__ __launch_bounds__(TGT_KTH_BLOCK) void tgt_kth_kernel(const float* __restrict__ points, TgtLevels lv,
                                                                const int32_t* __restrict__ level_live,
                                                                const float* __restrict__ boxes, const float* __restrict__ cs,
                                                                int m_cap, const int32_t* __restrict__ m_live,
                                                                const int32_t* __restrict__ counts, int limit, int topk,
                                                                int32_t* __restrict__ best, float* __restrict__ kth) {
  __shared__ unsigned hist[256];
  __shared__ int s_best, s_k;
  __shared__ unsigned s_prefix;
  const int j = blockIdx.x;
  if (j >= tgt_box_count(m_live, m_cap)) return;
  if (threadIdx.x == 0) {
    int b = lv.n - 1;                                    // no level has fewer than `limit`: the last one
    for (int l = 0; l < lv.n; ++l)
      if (counts[l * m_cap + j] < limit) { b = l > 0 ? l - 1 : 0; break; }
    int64_t n = 0;
    for (int l = 0; l < lv.n; ++l) n += tgt_level_live(lv, level_live, l);
    const int k = (int)(n < (int64_t)topk + 1 ? n : (int64_t)topk + 1);
    s_best = b;
    s_k = (k >= 1 && counts[b * m_cap + j] >= k) ? k : 0;
    s_prefix = 0u;
  }
  __syncthreads();
  const int b = s_best;
  int remaining = s_k;
  if (remaining == 0) {                                   // fewer candidates than k: the k-th entry is a non-candidate's -1
    if (threadIdx.x == 0) { best[j] = b; kth[j] = -1.0f; }
    return;
  }
  const int row0 = lv.start[b], row1 = row0 + tgt_level_live(lv, level_live, b);
  const float* bx = boxes + 7 * j;
  const float* rot = cs + 2 * j;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix;
    for (int row = row0 + (int)threadIdx.x; row < row1; row += TGT_KTH_BLOCK) {
      float t[6];
      if (!tgt_faces(points[3 * (int64_t)row], points[3 * (int64_t)row + 1], points[3 * (int64_t)row + 2], bx, rot, t)) continue;
      const unsigned bits = __float_as_uint(tgt_centerness(t));
      if (shift == 24 || (bits >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int acc = 0, bin = 0;
      for (int h = 255; h >= 0; --h) {
        const int c = (int)hist[h];
        if (acc + c >= remaining) { bin = h; break; }
        acc += c;
      }
      s_k = remaining - acc;                              // rank inside the chosen bin
      s_prefix = prefix | ((unsigned)bin << shift);
    }
    __syncthreads();
    remaining = s_k;
  }
  if (threadIdx.x == 0) { best[j] = b; kth[j] = __uint_as_float(s_prefix); }
}

// ---- assign: per row the smallest-volume box among those passing conditions 1-3 (ties: the lowest box index) -------------------
template <typename LabelT>
__global__ __launch_bounds__(TGT_BLOCK) void tgt_assign_kernel(const float* __restrict__ points, TgtLevels lv,
                                                               const int32_t* __restrict__ level_live,
                                                               const float* __restrict__ boxes, const float* __restrict__ cs,
                                                               const float* __restrict__ volume,
                                                               const LabelT* __restrict__ gt_label, int m_cap,
                                                               const int32_t* __restrict__ m_live,
                                                               const int32_t* __restrict__ best, const float* __restrict__ kth,
                                                               int32_t* __restrict__ labels, int32_t* __restrict__ row_box,
                                                               float* __restrict__ row_ctr, int32_t* __restrict__ block_cnt) {
  __shared__ int s_wave[TGT_BLOCK / 64];
  const int m = tgt_box_count(m_live, m_cap);
  const int l = tgt_level_of_block(lv, blockIdx.x);
  const int first = lv.start[l] + ((int)blockIdx.x - lv.block0[l]) * TGT_BLOCK;
  const int live_end = lv.start[l] + tgt_level_live(lv, level_live, l);
  const int row = first + threadIdx.x;
  const bool in_cap = row < lv.start[l + 1];
  const bool alive = row < live_end;
  int arg = -1;
  float ctr = 0.f;
  if (first < live_end) {                                  // uniform over the block
    float px = 0.f, py = 0.f, pz = 0.f;
    if (alive) { px = points[3 * (int64_t)row]; py = points[3 * (int64_t)row + 1]; pz = points[3 * (int64_t)row + 2]; }
    float best_vol = TGT_BIG_VOLUME;
    for (int j = 0; j < m; ++j) {
      if (best[j] != l) continue;                          // condition 2 (uniform)
      float t[6];
      if (!tgt_faces(px, py, pz, boxes + 7 * j, cs + 2 * j, t) || !alive) continue;          // condition 1
      const float cn = tgt_centerness(t);
      if (cn > kth[j] && volume[j] < best_vol) { best_vol = volume[j]; arg = j; ctr = cn; }   // condition 3, smallest volume
    }
  }
  if (in_cap) {
    labels[row] = arg >= 0 ? (int32_t)gt_label[arg] : -1;
    row_box[row] = arg;
    row_ctr[row] = ctr;
  }
  const unsigned long long bal = __ballot(arg >= 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < TGT_BLOCK / 64; ++w) c += s_wave[w];
    block_cnt[blockIdx.x] = c;
  }
}

// ---- scan: per-block positive counts -> exclusive offsets (in place), n_pos, and the rows of pos_* behind n_pos ------------------
__global__ __launch_bounds__(1024) void tgt_scan_kernel(int32_t* __restrict__ block_cnt, int n_blocks, int p_cap,
                                                        int32_t* __restrict__ pos_row, int32_t* __restrict__ pos_box,
                                                        float* __restrict__ pos_ctr, int32_t* __restrict__ n_pos) {
  __shared__ int smem[1024 / 64 + 1];
  int base = 0;
  for (int i0 = 0; i0 < n_blocks; i0 += 1024) {
    const int i = i0 + (int)threadIdx.x;
    const int v = i < n_blocks ? block_cnt[i] : 0;
    int total;
    const int excl = block_excl_scan<1024>(v, smem, &total);
    if (i < n_blocks) block_cnt[i] = base + excl;
    base += total;
  }
  const int np = base < p_cap ? base : p_cap;             // base <= m_live * topk <= p_cap: the clamp only guards the stores
  if (threadIdx.x == 0) n_pos[0] = np;
  for (int i = np + (int)threadIdx.x; i < p_cap; i += 1024) { pos_row[i] = 0; pos_box[i] = 0; pos_ctr[i] = 0.f; }
}

// ---- compact: the positive rows in ascending row order -------------------------------------------------------------------------
__global__ __launch_bounds__(TGT_BLOCK) void tgt_compact_kernel(TgtLevels lv, const int32_t* __restrict__ row_box,
                                                                const float* __restrict__ row_ctr,
                                                                const int32_t* __restrict__ block_off, int p_cap,
                                                                int32_t* __restrict__ pos_row, int32_t* __restrict__ pos_box,
                                                                float* __restrict__ pos_ctr) {
  __shared__ int smem[TGT_BLOCK / 64 + 1];
  const int l = tgt_level_of_block(lv, blockIdx.x);
  const int row = lv.start[l] + ((int)blockIdx.x - lv.block0[l]) * TGT_BLOCK + (int)threadIdx.x;
  const int arg = row < lv.start[l + 1] ? row_box[row] : -1;
  int total;
  const int slot = block_off[blockIdx.x] + block_excl_scan<TGT_BLOCK>(arg >= 0 ? 1 : 0, smem, &total);
  if (arg >= 0 && slot < p_cap) { pos_row[slot] = row; pos_box[slot] = arg; pos_ctr[slot] = row_ctr[row]; }
}

// workspace of the assignment: counts [8][m_cap] | best [m_cap] | kth [m_cap] | row_box [n_cap] | row_ctr [n_cap] | block_cnt
struct TgtWorkspace { size_t counts, best, kth, row_box, row_ctr, block_cnt, total; };
inline size_t tgt_align(size_t v) { return (v + 15) & ~(size_t)15; }
inline TgtWorkspace tgt_workspace(int64_t n_cap, int n_levels, int m_cap) {
  TgtWorkspace w;
  size_t o = 0;
  w.counts = o; o = tgt_align(o + sizeof(int32_t) * TGT_MAX_LEVELS * (size_t)m_cap);
  w.best = o; o = tgt_align(o + sizeof(int32_t) * (size_t)m_cap);
  w.kth = o; o = tgt_align(o + sizeof(float) * (size_t)m_cap);
  w.row_box = o; o = tgt_align(o + sizeof(int32_t) * (size_t)n_cap);
  w.row_ctr = o; o = tgt_align(o + sizeof(float) * (size_t)n_cap);
  w.block_cnt = o; o = tgt_align(o + sizeof(int32_t) * (size_t)(n_cap / TGT_BLOCK + n_levels + 1));
  w.total = o;
  return w;
}

inline bool tgt_levels(const int32_t* level_cap, int n_levels, TgtLevels* lv, int64_t* n_cap, int* n_blocks) {
  if (level_cap == nullptr || n_levels < 1 || n_levels > TGT_MAX_LEVELS) return false;
  int64_t rows = 0, blocks = 0;
  lv->n = n_levels;
  for (int l = 0; l <= TGT_MAX_LEVELS; ++l) {
    lv->start[l] = (int32_t)rows;
    lv->block0[l] = (int32_t)blocks;
    if (l < n_levels) {
      if (level_cap[l] < 0) return false;
      rows += level_cap[l];
      blocks += ceil_div(level_cap[l], TGT_BLOCK);
      if (rows > 0x7fffffff / 4) return false;             // 3 * row and the block arithmetic stay far inside int32
    }
  }
  *n_cap = rows;
  *n_blocks = (int)blocks;
  return true;
}

// ---- focal loss ---------------------------------------------------------------------------------------------------------------
// sum over live rows and classes of a_t (1 - p_t)^gamma BCE(x, t) (mmdet FocalLoss(use_sigmoid=True), un-normalised) and its
// derivative; t = (label == class), any label outside [0, n_cls) is a background row.  Element math in fp64; every block adds its
// elements in one fixed order into partial[block].
__global__ __launch_bounds__(TGT_BLOCK) void tgt_focal_kernel(const float* __restrict__ cls, const int32_t* __restrict__ labels,
                                                              TgtLevels lv, const int32_t* __restrict__ level_live, int n_cls,
                                                              int64_t n_elem, double gamma, double alpha,
                                                              float* __restrict__ grad, double* __restrict__ partial) {
  __shared__ double sm[TGT_BLOCK / 64];
  int live_end[TGT_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < TGT_MAX_LEVELS; ++l) live_end[l] = l < lv.n ? lv.start[l] + tgt_level_live(lv, level_live, l) : 0;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * TGT_BLOCK + threadIdx.x; i < n_elem; i += (int64_t)gridDim.x * TGT_BLOCK) {
    const int row = (int)(i / n_cls), c = (int)(i - (int64_t)row * n_cls);
    bool alive = false;
#pragma unroll
    for (int l = 0; l < TGT_MAX_LEVELS; ++l) alive = alive || (l < lv.n && row >= lv.start[l] && row < live_end[l]);
    float g = 0.f;
    if (alive) {
      const double x = (double)cls[i];
      const bool t = labels[row] == c;
      const double e = exp(-fabs(x)), d = 1.0 + e;
      const double p = x >= 0.0 ? 1.0 / d : e / d;        // sigmoid(x)
      const double q = x >= 0.0 ? e / d : 1.0 / d;        // 1 - sigmoid(x), without the cancellation
      const double bce = fmax(x, 0.0) - (t ? x : 0.0) + log1p(e);
      const double pt = t ? q : p, dpt = t ? -p * q : p * q, a = t ? alpha : 1.0 - alpha;
      double w, dw;                                       // pt^gamma and its derivative by pt
      if (gamma == 2.0) { w = pt * pt; dw = 2.0 * pt; }
      else if (gamma == 1.0) { w = pt; dw = 1.0; }
      else if (gamma == 0.0) { w = 1.0; dw = 0.0; }
      else { w = pow(pt, gamma); dw = gamma * pow(pt, gamma - 1.0); }
      s += a * w * bce;
      g = (float)(a * (dw * dpt * bce + w * (p - (t ? 1.0 : 0.0))));
    }
    grad[i] = g;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// out[c] = (float) sum_i in[c][i], c < n_cols, in one fixed order (one workgroup)
__global__ __launch_bounds__(TGT_BLOCK) void tgt_sum_columns_kernel(const double* __restrict__ in, int64_t n, int n_cols,
                                                                    float* __restrict__ out) {
  __shared__ double sm[TGT_BLOCK / 64];
  for (int c = 0; c < n_cols; ++c) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += TGT_BLOCK) s += in[(int64_t)c * n + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] = (float)((sm[0] + sm[1]) + (sm[2] + sm[3]));
    __syncthreads();
  }
}

// ---- forward-mode duals: a value and its derivatives by the seven parameters of the decoded box ---------------------------------
constexpr int ND = 7;
struct Dual {
  double v, d[ND];
};
__device__ __forceinline__ Dual dconst(double v) { Dual r; r.v = v; for (int k = 0; k < ND; ++k) r.d[k] = 0.0; return r; }
__device__ __forceinline__ Dual dvar(double v, int k) { Dual r = dconst(v); r.d[k] = 1.0; return r; }
__device__ __forceinline__ Dual operator+(const Dual& a, const Dual& b) { Dual r; r.v = a.v + b.v; for (int k = 0; k < ND; ++k) r.d[k] = a.d[k] + b.d[k]; return r; }
__device__ __forceinline__ Dual operator-(const Dual& a, const Dual& b) { Dual r; r.v = a.v - b.v; for (int k = 0; k < ND; ++k) r.d[k] = a.d[k] - b.d[k]; return r; }
__device__ __forceinline__ Dual operator*(const Dual& a, const Dual& b) { Dual r; r.v = a.v * b.v; for (int k = 0; k < ND; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k]; return r; }
__device__ __forceinline__ Dual operator/(const Dual& a, const Dual& b) {
  Dual r; r.v = a.v / b.v;
  for (int k = 0; k < ND; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
  return r;
}
__device__ __forceinline__ Dual operator+(const Dual& a, double b) { Dual r = a; r.v += b; return r; }
__device__ __forceinline__ Dual operator-(const Dual& a, double b) { Dual r = a; r.v -= b; return r; }
__device__ __forceinline__ Dual operator*(const Dual& a, double b) { Dual r; r.v = a.v * b; for (int k = 0; k < ND; ++k) r.d[k] = a.d[k] * b; return r; }
__device__ __forceinline__ Dual dneg(const Dual& a) { return a * -1.0; }
__device__ __forceinline__ Dual dclamp_min(const Dual& a, double lo) { return a.v >= lo ? a : dconst(lo); }   // torch.clamp: gradient where x >= min
__device__ __forceinline__ Dual dmin_c(const Dual& a, double b) { return a.v <= b ? a : dconst(b); }
__device__ __forceinline__ Dual dmax_c(const Dual& a, double b) { return a.v >= b ? a : dconst(b); }

struct DP { Dual x, y; };
struct P2d { double x, y; };
__device__ __forceinline__ Dual dcross(const DP& a, const DP& b) { return a.x * b.y - a.y * b.x; }

// IoU of the axis-aligned boxes pred (variables 0..5) and tgt (_IoU3DLoss.forward, with_yaw=False)
__device__ Dual tgt_iou_aligned(const double* a, const double* b) {
  Dual inter = dconst(1.0);
  for (int k = 0; k < 3; ++k) {
    const Dual c = dvar(a[k], k), h = dvar(a[3 + k], 3 + k) * 0.5;
    const Dual hi = dmin_c(c + h, b[k] + b[3 + k] / 2), lo = dmax_c(c - h, b[k] - b[3 + k] / 2);
    inter = inter * dclamp_min(hi - lo, 0.0);
  }
  const Dual uni = dvar(a[3], 3) * dvar(a[4], 4) * dvar(a[5], 5) + b[3] * b[4] * b[5] - inter;
  return inter / dclamp_min(uni, 1e-8);
}

// bird's-eye-view corners of the predicted box as duals (core/rotated_iou.py bev_corners), counter-clockwise
__device__ __forceinline__ DP tgt_corner_dual(const double* a, int i) {
  const double sx = (i == 0 || i == 3) ? 0.5 : -0.5, sy = i < 2 ? 0.5 : -0.5;
  const Dual lx = dvar(a[3], 3) * sx, ly = dvar(a[4], 4) * sy;
  Dual c = dconst(cos(a[6])), s = dconst(sin(a[6]));
  c.d[6] = -s.v; s.d[6] = c.v;
  DP r;
  r.x = lx * c - ly * s + dvar(a[0], 0);
  r.y = lx * s + ly * c + dvar(a[1], 1);
  return r;
}
__device__ __forceinline__ P2d tgt_corner(const double* b, int i) {
  const double lx = ((i == 0 || i == 3) ? 0.5 : -0.5) * b[3], ly = (i < 2 ? 0.5 : -0.5) * b[4];
  const double c = cos(b[6]), s = sin(b[6]);
  return P2d{lx * c - ly * s + b[0], lx * s + ly * c + b[1]};
}
__device__ __forceinline__ DP dpoint(const P2d& p) { DP r; r.x = dconst(p.x); r.y = dconst(p.y); return r; }

// candidate vertex `idx` of the intersection polygon (bev_intersection): 0..15 = crossing of edge idx/4 of the predicted box with
// edge idx%4 of the target, 16..19 = corners of the predicted box, 20..23 = corners of the target
__device__ DP tgt_vertex_dual(const double* a, const P2d* c2, int idx) {
  if (idx >= 20) return dpoint(c2[idx - 20]);
  if (idx >= 16) return tgt_corner_dual(a, idx - 16);
  const int i = idx >> 2, j = idx & 3;
  const DP p1 = tgt_corner_dual(a, i), p2 = tgt_corner_dual(a, (i + 1) & 3);
  const P2d p3 = c2[j], p4 = c2[(j + 1) & 3];
  DP d12, d34, r31;
  d12.x = p2.x - p1.x; d12.y = p2.y - p1.y;
  d34 = dpoint(P2d{p4.x - p3.x, p4.y - p3.y});
  r31.x = dneg(p1.x) + p3.x; r31.y = dneg(p1.y) + p3.y;
  const Dual t = dcross(r31, d34) / dcross(d12, d34);
  DP r;
  r.x = p1.x + t * d12.x;
  r.y = p1.y + t * d12.y;
  return r;
}

__device__ __forceinline__ bool tgt_in_rect(const P2d& p, const P2d* r) {
  const double eps = 1e-9;
  const double abx = r[1].x - r[0].x, aby = r[1].y - r[0].y, adx = r[3].x - r[0].x, ady = r[3].y - r[0].y;
  const double apx = p.x - r[0].x, apy = p.y - r[0].y;
  const double pab = apx * abx + apy * aby, pad = apx * adx + apy * ady;
  return pab >= -eps && pab <= abx * abx + aby * aby + eps && pad >= -eps && pad <= adx * adx + ady * ady + eps;
}

// IoU of the boxes pred (variables 0..6) and tgt, both rotated about z (core/rotated_iou.py rotated_iou_3d): the 16 edge
// crossings and the 8 contained corners in angular order around their centroid, shoelace.  Values first (which candidates are
// vertices and in which order), then the duals of the vertices in that order: a candidate that is no vertex adds no area and
// no derivative (the reference collapses it onto the first vertex).
__device__ Dual tgt_iou_rotated(const double* a, const double* b) {
  P2d c1[4], c2[4], v[24];
  bool ok[24];
  for (int i = 0; i < 4; ++i) { c1[i] = tgt_corner(a, i); c2[i] = tgt_corner(b, i); }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const P2d p1 = c1[i], p2 = c1[(i + 1) & 3], p3 = c2[j], p4 = c2[(j + 1) & 3];
      const double d12x = p2.x - p1.x, d12y = p2.y - p1.y, d34x = p4.x - p3.x, d34y = p4.y - p3.y;
      double den = d12x * d34y - d12y * d34x;
      const bool fine = fabs(den) > 1e-12;
      den = fine ? den : 1.0;
      const double rx = p3.x - p1.x, ry = p3.y - p1.y;
      const double t = (rx * d34y - ry * d34x) / den, u = (rx * d12y - ry * d12x) / den;
      ok[4 * i + j] = fine && t > 0.0 && t < 1.0 && u > 0.0 && u < 1.0;
      v[4 * i + j] = P2d{p1.x + t * d12x, p1.y + t * d12y};
    }
  for (int i = 0; i < 4; ++i) {
    v[16 + i] = c1[i]; ok[16 + i] = tgt_in_rect(c1[i], c2);
    v[20 + i] = c2[i]; ok[20 + i] = tgt_in_rect(c2[i], c1);
  }
  int n = 0;
  double mx = 0.0, my = 0.0;
  for (int i = 0; i < 24; ++i)
    if (ok[i]) { ++n; mx += v[i].x; my += v[i].y; }
  Dual area = dconst(0.0);
  if (n >= 3) {
    mx /= n; my /= n;
    int ord[24];
    double ang[24];
    int cnt = 0;
    for (int i = 0; i < 24; ++i) {
      if (!ok[i]) continue;
      const double w = atan2(v[i].y - my, v[i].x - mx);
      int p = cnt++;
      while (p > 0 && ang[p - 1] > w) { ang[p] = ang[p - 1]; ord[p] = ord[p - 1]; --p; }
      ang[p] = w; ord[p] = i;
    }
    const DP first = tgt_vertex_dual(a, c2, ord[0]);
    DP prev = first;
    Dual acc = dconst(0.0);
    for (int k = 1; k < n; ++k) {
      const DP cur = tgt_vertex_dual(a, c2, ord[k]);
      acc = acc + dcross(prev, cur);
      prev = cur;
    }
    acc = acc + dcross(prev, first);
    area = acc * (acc.v > 0.0 ? 0.5 : (acc.v < 0.0 ? -0.5 : 0.0));
  }
  const Dual cz = dvar(a[2], 2), hz = dvar(a[5], 5) * 0.5;
  const Dual zl = dmax_c(cz - hz, b[2] - b[5] / 2), zh = dmin_c(cz + hz, b[2] + b[5] / 2);
  const Dual iv = area * dclamp_min(zh - zl, 0.0);
  const Dual uni = dvar(a[3], 3) * dvar(a[4], 4) * dvar(a[5], 5) + b[3] * b[4] * b[5] - iv;
  return iv / dclamp_min(uni, 1e-8);
}

// ---- positive rows: centerness BCE and IoU3D loss, one thread per row of the P_cap block ---------------------------------------
// rows [n_pos, P_cap) are dead: zero gradients, zero contributions, inputs not read
__global__ __launch_bounds__(64) void tgt_positive_kernel(const float* __restrict__ logit, const float* __restrict__ pred, int W,
                                                          int rotated, const float* __restrict__ boxes,
                                                          const int32_t* __restrict__ pos_box, const float* __restrict__ pos_ctr,
                                                          const int32_t* __restrict__ n_pos, int p_cap, int m_cap,
                                                          float* __restrict__ grad_logit, float* __restrict__ grad_pred,
                                                          double* __restrict__ terms) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p_cap) return;
  int np = n_pos[0];
  np = np < 0 ? 0 : (np < p_cap ? np : p_cap);
  double bce = 0.0, iou_loss = 0.0, ctr = 0.0, g_logit = 0.0, g[ND];
  for (int k = 0; k < ND; ++k) g[k] = 0.0;
  if (i < np) {
    ctr = (double)pos_ctr[i];
    const double x = (double)logit[i];
    const double e = exp(-fabs(x));
    bce = fmax(x, 0.0) - x * ctr + log1p(e);
    g_logit = (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - ctr;
    int j = pos_box[i];
    j = j < 0 ? 0 : (j < m_cap ? j : m_cap - 1);
    double a[7], b[7];
    for (int k = 0; k < 7; ++k) { a[k] = k < W ? (double)pred[(int64_t)i * W + k] : 0.0; b[k] = (double)boxes[7 * j + k]; }
    const Dual iou = rotated ? tgt_iou_rotated(a, b) : tgt_iou_aligned(a, b);
    iou_loss = (1.0 - iou.v) * ctr;
    for (int k = 0; k < ND; ++k) g[k] = -iou.d[k] * ctr;
  }
  grad_logit[i] = (float)g_logit;
  for (int k = 0; k < W; ++k) grad_pred[(int64_t)i * W + k] = (float)g[k];
  terms[i] = bce;
  terms[(int64_t)p_cap + i] = iou_loss;
  terms[2 * (int64_t)p_cap + i] = ctr;
}

constexpr int TGT_FOCAL_MAX_BLOCKS = 4096;
inline int tgt_focal_blocks(int64_t n_elem) {
  const int64_t b = ceil_div(n_elem, TGT_BLOCK);
  return (int)(b < 1 ? 1 : (b > TGT_FOCAL_MAX_BLOCKS ? TGT_FOCAL_MAX_BLOCKS : b));
}

}  // namespace

extern "C" size_t cnrma_fcaf3d_assign_workspace_bytes(int64_t n_cap, int n_levels, int m_cap) {
  if (n_cap < 0 || n_cap > 0x7fffffff / 4 || n_levels < 1 || n_levels > TGT_MAX_LEVELS || m_cap < 1 || m_cap > TGT_MAX_BOXES)
    return 0;
  return tgt_workspace(n_cap, n_levels, m_cap).total;
}

extern "C" int cnrma_fcaf3d_assign_f32(const float* points, const int32_t* level_cap, int n_levels, const int32_t* level_live,
                                       const float* boxes, const float* cs, const float* volume, const void* gt_label,
                                       int label_is_i64, int m_cap, const int32_t* m_live, int limit, int topk,
                                       void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* pos_row,
                                       int32_t* pos_box, float* pos_ctr, int32_t* n_pos, void* stream) {
  TgtLevels lv;
  int64_t n_cap = 0;
  int n_blocks = 0;
  if (!tgt_levels(level_cap, n_levels, &lv, &n_cap, &n_blocks)) return CNRMA_EINVAL;
  if (m_cap < 1 || m_cap > TGT_MAX_BOXES || topk < 1 || topk > 65536 || limit < 0 || m_live == nullptr || boxes == nullptr ||
      cs == nullptr || volume == nullptr || gt_label == nullptr || pos_row == nullptr || pos_box == nullptr ||
      pos_ctr == nullptr || n_pos == nullptr || (n_cap > 0 && (points == nullptr || labels == nullptr)))
    return CNRMA_EINVAL;
  const TgtWorkspace w = tgt_workspace(n_cap, n_levels, m_cap);
  if (workspace == nullptr || workspace_bytes < w.total || ((uintptr_t)workspace & 15) != 0) return CNRMA_EINVAL;
  char* ws = static_cast<char*>(workspace);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + w.counts);
  int32_t* best = reinterpret_cast<int32_t*>(ws + w.best);
  float* kth = reinterpret_cast<float*>(ws + w.kth);
  int32_t* row_box = reinterpret_cast<int32_t*>(ws + w.row_box);
  float* row_ctr = reinterpret_cast<float*>(ws + w.row_ctr);
  int32_t* block_cnt = reinterpret_cast<int32_t*>(ws + w.block_cnt);
  const int p_cap = m_cap * topk;
  hipStream_t st = as_stream(stream);
  hipError_t e = cnrma_fill_bytes(counts, 0, w.best - w.counts, st);
  if (e != hipSuccess) return -(int)e;
  if (n_blocks > 0) {
    hipLaunchKernelGGL(tgt_count_kernel, dim3(n_blocks), dim3(TGT_BLOCK), sizeof(int32_t) * m_cap, st, points, lv, level_live,
                       boxes, cs, m_cap, m_live, counts);
    CNRMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tgt_kth_kernel, dim3(m_cap), dim3(TGT_KTH_BLOCK), 0, st, points, lv, level_live, boxes, cs, m_cap, m_live,
                     counts, limit, topk, best, kth);
  CNRMA_LAUNCH_CHECK();
  if (n_blocks > 0) {
    if (label_is_i64)
      hipLaunchKernelGGL(tgt_assign_kernel<int64_t>, dim3(n_blocks), dim3(TGT_BLOCK), 0, st, points, lv, level_live, boxes, cs,
                         volume, static_cast<const int64_t*>(gt_label), m_cap, m_live, best, kth, labels, row_box, row_ctr,
                         block_cnt);
    else
      hipLaunchKernelGGL(tgt_assign_kernel<int32_t>, dim3(n_blocks), dim3(TGT_BLOCK), 0, st, points, lv, level_live, boxes, cs,
                         volume, static_cast<const int32_t*>(gt_label), m_cap, m_live, best, kth, labels, row_box, row_ctr,
                         block_cnt);
    CNRMA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(tgt_scan_kernel, dim3(1), dim3(1024), 0, st, block_cnt, n_blocks, p_cap, pos_row, pos_box, pos_ctr, n_pos);
  CNRMA_LAUNCH_CHECK();
  if (n_blocks > 0) {
    hipLaunchKernelGGL(tgt_compact_kernel, dim3(n_blocks), dim3(TGT_BLOCK), 0, st, lv, row_box, row_ctr, block_cnt, p_cap,
                       pos_row, pos_box, pos_ctr);
    CNRMA_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" size_t cnrma_fcaf3d_focal_loss_workspace_bytes(int64_t n_cap, int n_cls) {
  if (n_cap < 0 || n_cls < 1) return 0;
  return sizeof(double) * (size_t)tgt_focal_blocks(n_cap * n_cls);
}

extern "C" int cnrma_fcaf3d_focal_loss_f32(const float* cls, const int32_t* labels, const int32_t* level_cap, int n_levels,
                                           const int32_t* level_live, int n_cls, float gamma, float alpha, void* workspace,
                                           size_t workspace_bytes, float* loss_sum, float* grad_cls, void* stream) {
  TgtLevels lv;
  int64_t n_cap = 0;
  int n_blocks = 0;
  if (!tgt_levels(level_cap, n_levels, &lv, &n_cap, &n_blocks)) return CNRMA_EINVAL;
  if (n_cls < 1 || n_cls > 65535 || loss_sum == nullptr || (n_cap > 0 && (cls == nullptr || labels == nullptr || grad_cls == nullptr)))
    return CNRMA_EINVAL;
  const int64_t n_elem = n_cap * n_cls;
  const int blocks = tgt_focal_blocks(n_elem);
  if (workspace == nullptr || workspace_bytes < sizeof(double) * (size_t)blocks || ((uintptr_t)workspace & 7) != 0)
    return CNRMA_EINVAL;
  double* partial = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tgt_focal_kernel, dim3(blocks), dim3(TGT_BLOCK), 0, st, cls, labels, lv, level_live, n_cls, n_elem,
                     (double)gamma, (double)alpha, grad_cls, partial);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(tgt_sum_columns_kernel, dim3(1), dim3(TGT_BLOCK), 0, st, partial, (int64_t)blocks, 1, loss_sum);
  CNRMA_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cnrma_fcaf3d_positive_losses_workspace_bytes(int p_cap) {
  return p_cap < 1 ? 0 : sizeof(double) * 3 * (size_t)p_cap;
}

extern "C" int cnrma_fcaf3d_positive_losses_f32(const float* logit, const float* pred_boxes, int box_cols, int rotated,
                                                const float* boxes, int m_cap, const int32_t* pos_box, const float* pos_ctr,
                                                const int32_t* n_pos, int p_cap, void* workspace, size_t workspace_bytes,
                                                float* sums, float* grad_logit, float* grad_boxes, void* stream) {
  if (p_cap < 1 || m_cap < 1 || (box_cols != 6 && box_cols != 7) || (rotated != 0 && box_cols != 7) || logit == nullptr ||
      pred_boxes == nullptr || boxes == nullptr || pos_box == nullptr || pos_ctr == nullptr || n_pos == nullptr ||
      sums == nullptr || grad_logit == nullptr || grad_boxes == nullptr)
    return CNRMA_EINVAL;
  if (workspace == nullptr || workspace_bytes < sizeof(double) * 3 * (size_t)p_cap || ((uintptr_t)workspace & 7) != 0)
    return CNRMA_EINVAL;
  double* terms = static_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(tgt_positive_kernel, dim3((unsigned)ceil_div(p_cap, 64)), dim3(64), 0, st, logit, pred_boxes, box_cols,
                     rotated, boxes, pos_box, pos_ctr, n_pos, p_cap, m_cap, grad_logit, grad_boxes, terms);
  CNRMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(tgt_sum_columns_kernel, dim3(1), dim3(TGT_BLOCK), 0, st, terms, (int64_t)p_cap, 3, sums);
  CNRMA_LAUNCH_CHECK();
  return 0;
}
