"""Generator of the volume-bounds fixtures (not collected by pytest; run in the build container, where the reference is mounted):

    python tests/golden/make_golden_bounds.py            # writes bounds_general.npz and bounds_edge.npz beside this file

It imports the reference's depth_to_world (data_prepare/scannet/tsdf.py:77-101, loaded from where it lies by make_golden_fusion's
load_reference -- tests/golden/_ref_import.py loads the projects/ tree, which has no depth_to_world), runs it on the CPU frame by frame the
way generate_tsdf.py:82-101 does -- mask, back-project, concatenate, keep the rows with a finite x, np.quantile --
beside tests/bounds_oracle.py, and asserts bit equality of the points, the kept mask, the quantiles, the origin and voxel_dim, and that
each named edge case occurs.  No reference source is copied: only what its function computes is saved.  The archives are written with
a fixed time stamp, so running the generator again reproduces them byte for byte."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import bounds_oracle as BO  # noqa: E402
from make_golden_fusion import bits_equal, load_reference, save_npz  # noqa: E402


def load_depth_to_world():
    return load_reference().depth_to_world


def camera(eye, target, focal, cx, cy):
    """-> (3x4 projection K [R | t] float32, R) of a camera at `eye` looking at `target`, world z up, image y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    R = np.stack((r, np.cross(f, r), f))
    K = np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1.0]])
    return (K @ np.concatenate((R, (-R @ eye)[:, None]), axis=1)).astype(np.float32), R


def run_case(depth_to_world, name, proj, depth, voxel_size, max_depth, vol_prcnt, vol_margin):
    """the reference's lines beside the oracle -> arrays to save"""
    proj, depth = torch.from_numpy(proj), torch.from_numpy(depth)
    ref_pts, own_pts, pinv = [], [], []
    for v in range(len(proj)):
        d = depth[v].clone()
        if max_depth is not None:
            d[d > max_depth] = 0                                         # generate_tsdf.py:94
        ref_pts.append(depth_to_world(proj[v], d).view(3, -1).T)
        pinv.append(BO.inverse_projection(proj[v]))
        own_pts.append(BO.back_project(pinv[-1], BO.mask_depth(depth[v], max_depth)).T)
    ref_pts, own_pts = torch.cat(ref_pts), torch.cat(own_pts)
    ref_kept, own_kept = torch.isfinite(ref_pts[:, 0]), torch.isfinite(own_pts[:, 0])
    assert torch.equal(ref_kept, own_kept), (name, "kept mask")
    assert torch.equal(torch.isfinite(ref_pts), torch.isfinite(own_pts)), (name, "finiteness")
    pts = ref_pts[ref_kept].numpy()
    assert bits_equal(pts, own_pts[own_kept].numpy()), (name, "points")
    assert bits_equal(pts, BO.cloud(proj, depth, max_depth)), (name, "cloud")
    low, high = np.quantile(pts, 1 - vol_prcnt, axis=0), np.quantile(pts, vol_prcnt, axis=0)
    origin = torch.as_tensor(low - vol_margin).float()
    vol_max = torch.as_tensor(high + vol_margin).float()
    voxel_dim = ((vol_max - origin) / voxel_size).int().tolist()
    own_origin, own_dim, own_q = BO.bounds(proj, depth, voxel_size, max_depth, vol_prcnt, vol_margin)
    assert bits_equal(np.stack((low, high)), own_q) and bits_equal(origin.numpy(), own_origin.numpy()) and voxel_dim == own_dim, name
    values, counts = BO.order_statistics(pts, 1 - vol_prcnt, vol_prcnt)
    assert low.dtype == np.float32 and counts[0] == len(pts)
    return dict(proj=proj.numpy(), depth=depth.numpy(), pinv=torch.stack(pinv).numpy(), voxel_size=np.float64(voxel_size),
                max_depth=np.float64(np.inf if max_depth is None else max_depth), vol_prcnt=np.float64(vol_prcnt),
                vol_margin=np.float64(vol_margin), n=np.int64(len(pts)), quantiles=own_q, origin=origin.numpy(),
                voxel_dim=np.asarray(voxel_dim, np.int64), values=values, counts=counts), pts


def general_case(depth_to_world):
    """three cameras inside a room of 4 x 5 x 2.5 m, 24 x 32 pixels each: the depth of its walls with noise, far walls beyond max_depth =
    3, rectangles of 0, -1, NaN and +inf depth"""
    rng = np.random.default_rng(20240917)
    H, W, focal = 24, 32, 26.0
    lo, hi = np.array([-2.0, -2.5, 0.0]), np.array([2.0, 2.5, 2.5])
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack(((u - W / 2) / focal, (v - H / 2) / focal, np.ones_like(u)), axis=-1)
    proj, depth = [], []
    for eye, target in (((-0.9, -1.4, 1.3), (1.6, 2.0, 0.9)), ((1.1, 0.4, 1.5), (-2.0, -1.0, 0.4)), ((0.2, 1.6, 1.1), (0.6, -2.5, 1.6))):
        P, R = camera(eye, target, focal, W / 2, H / 2)
        d = rays @ R                                                     # world direction per unit of camera depth
        with np.errstate(divide="ignore"):
            t = np.where(d > 0, (hi - eye) / d, (lo - eye) / d)
        proj.append(P)
        depth.append(t.min(-1) + rng.normal(0, 0.01, (H, W)))
    proj, depth = np.stack(proj), np.stack(depth).astype(np.float32)
    depth[:, 2:5, 3:9] = 0.0
    depth[:, 7:10, 12:18] = -1.0
    depth[:, 13:16, 20:26] = np.nan
    depth[:, 18:21, 5:11] = np.inf
    arrays, pts = run_case(depth_to_world, "general", proj, depth, 0.04, 3.0, 0.995, 1.5)
    finite = depth[np.isfinite(depth)]
    assert (finite > 3.0).sum() > 100 and ((finite > 0) & (finite <= 3.0)).sum() > 500
    assert len(pts) == ((depth <= 3.0) & (depth != 0)).sum()             # negative depths are kept; 0, NaN, inf and far ones are not
    last_row = arrays["pinv"][:, 3]
    assert (last_row != np.array([0, 0, 0, 1], np.float32)).any()        # the inverse's last row is not exactly 0 0 0 1
    print(f"general: {len(pts)} of {depth.size} pixels kept, origin {arrays['origin']}, voxel_dim {arrays['voxel_dim']}")
    return arrays


def edge_case(depth_to_world):
    """two cameras of 8 x 8 pixels, each given twice (views 0 1 0 1): every value occurs an even number of times, so every rank pair
    (k, k + 1) with k odd joins two different values.  All 256 pixels are kept.  192 of them lie within 2 m in front of the cameras,
    which stand at z = -2.5 (z < 0 there); the lower half of view 1 lies 50 m away (z > 0): with vol_prcnt = 0.75, k = 191 is the last
    point of the near cluster and k + 1 the first of the far one on z.  x and y change sign across each image."""
    rng = np.random.default_rng(5)
    H = W = 8
    proj = np.stack([camera((0.3, -0.2, -2.5), (0.6, 0.4, 5.0), 9.0, 3.5, 3.5)[0],
                     camera((-0.4, 0.1, -2.5), (0.1, 0.3, 5.0), 9.0, 3.5, 3.5)[0]])
    depth = rng.uniform(0.5, 2.0, (2, H, W)).astype(np.float32)
    depth[1, 4:] = rng.uniform(50.0, 60.0, (4, W)).astype(np.float32)
    proj, depth = np.concatenate((proj, proj)), np.concatenate((depth, depth))
    arrays, pts = run_case(depth_to_world, "edge", proj, depth, 0.04, None, 0.75, 1.5)
    n = len(pts)
    assert n == 256
    s = np.sort(pts, axis=0)
    assert (s[0::2] == s[1::2]).all()                                    # every value is a tie
    for q in (0.25, 0.75):
        k, k1 = BO.ranks(n, q)
        assert k % 2 == 1 and k1 == k + 1 and (s[k] != s[k1]).all(), (q, k, k1)
    k, k1 = BO.ranks(n, 0.75)
    assert k == 191 and s[k, 2] < 0 < 40 < s[k1, 2]
    assert BO.float_key(s[k, 2]) >> 24 != BO.float_key(s[k1, 2]) >> 24   # the pair straddles a border of the select's first digit
    assert all((s[:, a] < 0).any() and (s[:, a] > 0).any() for a in range(3))
    print(f"edge: {n} points, z ranks {k} / {k1}: {s[k, 2]} / {s[k1, 2]}, quantiles {arrays['quantiles'].tolist()}")
    return arrays


if __name__ == "__main__":
    fn = load_depth_to_world()
    for name, case in (("bounds_general", general_case), ("bounds_edge", edge_case)):
        path = os.path.join(HERE, name + ".npz")
        save_npz(path, case(fn))
        size = os.path.getsize(path)
        assert size < 100000, (name, size)
        print(f"{name}.npz: {size} bytes")
