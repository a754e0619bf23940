"""Host oracle of the TSDF fusion (cnrma_amd.fusion / csrc/fusion.hip): the arithmetic of include/cnrma.h (a16) restated in torch
on the CPU, one full-volume expression per step, every choice a torch.where.  tests/golden/make_golden_fusion.py asserts that it
equals the reference's TSDFFusion(device='cpu') bit for bit; the tests then use it wherever no fixture exists.

    state = fuse(dims, voxel_size, origin, proj, depth, color, label, trunc_ratio=3, max_depth=None, history=False)

Volumes are flat [N] (colour [3,N]), index (x Y + y) Z + z.  All arithmetic is float32."""
import torch

from oracle.rma_oracle import matmul_fma_chain


def initial_state(dims, color=True, label=False):
    n = dims[0] * dims[1] * dims[2]
    return dict(tsdf=torch.ones(n), weight=torch.zeros(n), color=torch.zeros(3, n) if color else None,
                label=torch.full((n,), -1, dtype=torch.int64) if label else None)


def world_points(dims, voxel_size, origin):
    """[4, N] float32: voxel index * voxel_size (rounded) + origin (rounded), and a row of ones"""
    X, Y, Z = dims
    g = torch.arange(X * Y * Z, dtype=torch.long)
    idx = torch.stack((g // (Y * Z), (g // Z) % Y, g % Z)).float()
    org = torch.as_tensor(origin, dtype=torch.float32).reshape(3, 1)
    world = idx * torch.tensor(voxel_size, dtype=torch.float32) + org
    return torch.cat((world, torch.ones_like(world[:1])), dim=0)


def integrate_view(state, world, trunc_margin, proj, depth, color=None, label=None, max_depth=None):
    """one view into `state` (a new dict; the old one is left as it was)"""
    H, W = depth.shape
    cam = matmul_fma_chain(proj.float(), world)
    px, py, pz = torch.round(cam[0] / cam[2]), torch.round(cam[1] / cam[2]), cam[2]
    ok = (px >= 0) & (px < W) & (py >= 0) & (py < H) & (pz > 0)
    ix, iy = torch.where(ok, px, torch.zeros_like(px)).long(), torch.where(ok, py, torch.zeros_like(py)).long()
    d = depth.float()[iy, ix]
    if max_depth is not None:
        d = torch.where(d > max_depth, torch.zeros_like(d), d)
    ok = ok & (d > 0)
    q = (pz - d) / torch.tensor(trunc_margin, dtype=torch.float32)           # trunc_margin: a Python float, rounded once
    dist = torch.where(q < -1, torch.full_like(q, -1.0), q)                  # a NaN stays a NaN and fails the next test
    ok = ok & (dist < 1)
    near = ok & (dist > -1)
    t, w = state["tsdf"], state["weight"]
    fresh = ok & (w == 0)
    out = dict(tsdf=torch.where(fresh, dist, torch.where(near, t + dist, t)), weight=torch.where(near, w + 1, w), color=None,
               label=None)
    if state["color"] is not None:
        out["color"] = torch.where(near.unsqueeze(0), state["color"] + color.float()[:, iy, ix], state["color"])
    if state["label"] is not None:
        out["label"] = torch.where(near, label.long()[iy, ix], state["label"])
    return out


def fuse(dims, voxel_size, origin, proj, depth, color=None, label=None, trunc_ratio=3, max_depth=None, state=None, history=False):
    """proj [V,3,4], depth [V,H,W], color [V,3,H,W] or None, label [V,H,W] or None, fused in index order from `state` (default:
    the initial one; a colour / label volume is kept when the images are given).  -> the final state, or with history=True the
    list of states after every view."""
    if state is None:
        state = initial_state(dims, color is not None, label is not None)
    world = world_points(dims, voxel_size, origin)
    trunc_margin = voxel_size * trunc_ratio
    states = []
    for v in range(proj.shape[0]):
        state = integrate_view(state, world, trunc_margin, proj[v], depth[v], None if state["color"] is None else color[v],
                               None if state["label"] is None else label[v], max_depth)
        states.append(state)
    return states if history else state


def finish(state):
    """get_tsdf: (tsdf, colour) with the sums divided by the weight where it is positive"""
    w = state["weight"]
    seen = w > 0
    safe = torch.where(seen, w, torch.ones_like(w))
    t = torch.where(seen, state["tsdf"] / safe, state["tsdf"])
    c = None if state["color"] is None else torch.where(seen.unsqueeze(0), state["color"] / safe, state["color"])
    return t, c
