// Bird's-eye-view geometry of (x, y, z, dx, dy, dz, heading) boxes, shared by nms.hip (suppression masks, the pairwise IoU matrix)
// and eval.hip (the mAP evaluation's best-box search): both translation units round every overlap through these functions.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct P2 { float x, y; };

__device__ __forceinline__ float cross2(P2 a, P2 b, P2 c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); }

// corners of a BEV rectangle (centre cx,cy, size dx,dy, heading a), counter-clockwise
__device__ __forceinline__ void bev_corners(const float* b, P2* c) {
  const float ca = cosf(b[6]), sa = sinf(b[6]);
  const float hx = b[3] * 0.5f, hy = b[4] * 0.5f;
  const float lx[4] = {hx, -hx, -hx, hx}, ly[4] = {hy, hy, -hy, -hy};
#pragma unroll
  for (int i = 0; i < 4; ++i) { c[i].x = b[0] + lx[i] * ca - ly[i] * sa; c[i].y = b[1] + lx[i] * sa + ly[i] * ca; }
}

// area of the intersection of two convex quadrilaterals (Sutherland-Hodgman clipping of A by the edges of B)
__device__ float quad_intersection_area(const P2* A, const P2* B) {
  P2 poly[10], tmp[10];
  int n = 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) poly[i] = A[i];
  for (int e = 0; e < 4 && n > 0; ++e) {
    const P2 p = B[e], q = B[(e + 1) & 3];
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const P2 s = poly[i], t = poly[(i + 1) % n];
      const float ds = cross2(p, q, s), dt = cross2(p, q, t);
      if (ds >= 0.0f) tmp[m++] = s;
      if ((ds > 0.0f && dt < 0.0f) || (ds < 0.0f && dt > 0.0f)) {
        const float u = ds / (ds - dt);
        tmp[m].x = s.x + u * (t.x - s.x);
        tmp[m].y = s.y + u * (t.y - s.y);
        ++m;
      }
    }
    n = m;
    for (int i = 0; i < n; ++i) poly[i] = tmp[i];
  }
  float area = 0.0f;
  for (int i = 0; i < n; ++i) { const P2 a = poly[i], b = poly[(i + 1) % n]; area += a.x * b.y - a.y * b.x; }
  return fabsf(area) * 0.5f;
}

// BEV overlap of two rotated boxes.  A box without area overlaps nothing: its edges have no length or its corners no interior,
// so every point passes the clipper's side test and the other box would come back whole.
// Sizes are taken to be >= 0: a box with two negative sizes is outside the contract and is not caught by the product test.
__device__ __forceinline__ float rotated_bev_intersection(const float* a, const float* b) {
  if (!(a[3] * a[4] > 0.0f) || !(b[3] * b[4] > 0.0f)) return 0.0f;
  P2 ca[4], cb[4];
  bev_corners(a, ca);
  bev_corners(b, cb);
  return quad_intersection_area(ca, cb);
}

// BEV overlap of two axis-aligned boxes (the heading is not read)
__device__ __forceinline__ float aligned_bev_intersection(const float* p, const float* q) {
  const float lx = fmaxf(p[0] - p[3] * 0.5f, q[0] - q[3] * 0.5f), rx = fminf(p[0] + p[3] * 0.5f, q[0] + q[3] * 0.5f);
  const float ly = fmaxf(p[1] - p[4] * 0.5f, q[1] - q[4] * 0.5f), ry = fminf(p[1] + p[4] * 0.5f, q[1] + q[4] * 0.5f);
  return fmaxf(rx - lx, 0.0f) * fmaxf(ry - ly, 0.0f);
}

// 3D IoU (BEV overlap x height overlap): the arithmetic of nms.hip's iou_matrix_kernel with mode3d = 1, operation for operation
__device__ __forceinline__ float box_iou3d(const float* p, const float* q, int rotated) {
  const float inter = rotated ? rotated_bev_intersection(p, q) : aligned_bev_intersection(p, q);
  const float zl = fmaxf(p[2] - p[5] * 0.5f, q[2] - q[5] * 0.5f), zh = fminf(p[2] + p[5] * 0.5f, q[2] + q[5] * 0.5f);
  const float iv = inter * fmaxf(zh - zl, 0.0f);
  const float uv = p[3] * p[4] * p[5] + q[3] * q[4] * q[5] - iv;
  return iv / fmaxf(uv, 1e-8f);
}

}  // namespace
