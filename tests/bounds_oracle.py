"""Host oracle of the fusion-volume bounds (cnrma_amd.fusion.scene_bounds / csrc/bounds.hip): the arithmetic of include/cnrma_prep.h
(p1) restated in torch and numpy on the CPU -- every depth pixel back-projected, the rows with a finite x kept, np.quantile over
them.  tests/golden/make_golden_bounds.py asserts that it equals the reference (depth_to_world and the lines of generate_tsdf.py
around it) bit for bit; the tests then use it wherever no fixture exists.

    pts = cloud(projections, depths, max_depth)                                  # [n, 3] float32 numpy: the kept points
    origin, voxel_dim, q = bounds(projections, depths, voxel_size, ...)          # float32 tensor [3], list of 3 ints, [2, 3] quantiles
    values, counts = order_statistics(pts, q_lo, q_hi)                           # what the C entry point delivers

All arithmetic is float32."""
import numpy as np
import torch

from oracle.rma_oracle import matmul_fma_chain


def inverse_projection(projection):
    """[4,4]: the inverse of the 3x4 projection with the row 0 0 0 1 under it, one matrix at a time, on the CPU"""
    bottom = torch.tensor([[0., 0., 0., 1.]])
    return torch.inverse(torch.cat((projection.float().cpu(), bottom)))


def mask_depth(depth, max_depth=None):
    depth = depth.float()
    return depth if max_depth is None else torch.where(depth > max_depth, torch.zeros_like(depth), depth)


def back_project(pinv, depth):
    """pinv [4,4], depth [H,W] (already masked) -> world points [3, H*W], pixel order: (column, row, 1, 1 / depth) through pinv as a
    chain of fused multiply-adds, then divided by the fourth row"""
    H, W = depth.shape
    rows, cols = torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32)
    pixel = torch.stack((cols.repeat(H), rows.repeat_interleave(W), torch.ones(H * W), 1 / depth.reshape(-1)))
    Q = matmul_fma_chain(pinv, pixel)
    return Q[:3] / Q[3:]


def cloud(projections, depths, max_depth=None, pinv=None):
    """the kept points of all views, [n, 3] float32 numpy, in view and pixel order; pinv [V,4,4] replaces the inverses when given"""
    rows = []
    for v in range(len(depths)):
        m = inverse_projection(projections[v]) if pinv is None else pinv[v]
        rows.append(back_project(m, mask_depth(depths[v], max_depth)).T)
    pts = torch.cat(rows) if rows else torch.zeros(0, 3)
    return pts[torch.isfinite(pts[:, 0])].numpy()


def bounds_of_cloud(pts, voxel_size, vol_prcnt=.995, vol_margin=1.5):
    """-> (origin float32 tensor [3], voxel_dim list, quantiles [2,3] float32) of a kept cloud [n,3]"""
    if len(pts) == 0:
        raise ValueError("no pixel with a usable depth")
    low, high = np.quantile(pts, 1 - vol_prcnt, axis=0), np.quantile(pts, vol_prcnt, axis=0)
    origin = torch.as_tensor(low - vol_margin).float()
    far = torch.as_tensor(high + vol_margin).float()
    return origin, ((far - origin) / voxel_size).int().tolist(), np.stack((low, high))


def bounds(projections, depths, voxel_size, max_depth=None, vol_prcnt=.995, vol_margin=1.5):
    return bounds_of_cloud(cloud(projections, depths, max_depth), voxel_size, vol_prcnt, vol_margin)


def ranks(n, q):
    """(k, k1): the two rows of the sorted sample that np.quantile (numpy 2, method 'linear') interpolates between for a float32
    sample of n rows and a Python-float q -- numpy takes q and the virtual index (n - 1) * q to float32"""
    vi = np.float32(n - 1) * np.float32(q)
    if vi >= np.float32(n - 1):
        return n - 1, n - 1
    k = np.floor(vi)
    return int(k), min(int(k + np.float32(1)), n - 1)


def float_key(x):
    """the order-preserving 32-bit key the device's radix select walks: negative floats bit-flipped, the others with the top bit set"""
    u = int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])
    return (~u & 0xFFFFFFFF) if u >> 31 else (u | 0x80000000)


def order_statistics(pts, q_lo, q_hi):
    """-> (values [2,3,2] float32: quantile, axis, (s[k], s[k1]); counts [4] int64: n and the NaNs per axis) of a kept cloud [n,3]"""
    n = len(pts)
    counts = np.array([n] + [int(np.isnan(pts[:, a]).sum()) for a in range(3)], np.int64)
    values = np.zeros((2, 3, 2), np.float32)
    if n:
        s = np.sort(pts, axis=0)
        for i, q in enumerate((q_lo, q_hi)):
            k, k1 = ranks(n, q)
            values[i, :, 0], values[i, :, 1] = s[k], s[k1]
    return values, counts
