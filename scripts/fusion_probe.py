"""Time of the device TSDF fusion (cnrma_amd.fusion / csrc/fusion.hip) per view: python scripts/fusion_probe.py [--out FILE.json]
[--reps R] [--views V]

Three ways to fuse the same V posed 480x640 depth + colour maps into the same volume, timed in the same run, alternating within
every repetition, each window closed by HIP events and holding all V views:
  single    V launches of cnrma_tsdf_fuse_f32 with one view each (the reference's calling pattern)
  batched   one launch with all V views (the volumes cross memory once)
  torch     the BASELINE: a torch restatement of the reference's per-frame integrate (data_prepare/scannet/tsdf.py:402-451: full-volume
            passes, masked gathers and scatters) on the same device, V calls.  Never the code under test.
Reports the median and minimum per-view time of each, the algorithmic bytes per launch (2 * 5 * 4 * N for the volumes -- read and
written once per launch, because a lane keeps its voxel in registers across the views -- plus 16 * H * W * V for the maps), their
time at 8 TB/s and the share of it reached, and whether the two expectations hold: batched <= single and single <= torch per view.
Also how many voxels of the torch baseline differ from the library's result, and by how much at most in the tsdf sum (on a
device torch divides by a host scalar through its reciprocal, so the last bit of dist may differ there; the pinned behaviour is
the reference on the CPU)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import _lib  # noqa: E402
from cnrma_amd.fusion import TSDFFusion  # noqa: E402

SHAPES = ((192, 192, 80), (192, 192, 192), (256, 256, 96))
H, W, FOCAL, VOXEL = 480, 640, 577.0, 0.04
HBM_BYTES_PER_S = 8e12


def make_views(dims, V, seed=0):
    """cameras on a ring inside the volume's footprint looking across it, depth 0.5 - 4.5 m in smooth patches with 5 % holes"""
    rng = np.random.default_rng(seed)
    ext = VOXEL * np.asarray(dims, np.float64)
    centre = 0.5 * ext
    proj = []
    for a in 2 * np.pi * np.arange(V) / V:
        eye = centre + [0.3 * ext[0] * np.cos(a), 0.3 * ext[1] * np.sin(a), 0.1 * ext[2]]
        target = centre - [0.3 * ext[0] * np.cos(a), 0.3 * ext[1] * np.sin(a), 0.1 * ext[2]]
        f = (target - eye) / np.linalg.norm(target - eye)
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        R = np.stack((r, np.cross(f, r), f))
        K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1.0]])
        proj.append(K @ np.concatenate((R, (-R @ eye)[:, None]), axis=1))
    coarse = torch.from_numpy(rng.uniform(0.5, 4.5, (V, 1, 15, 20)).astype(np.float32))
    depth = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0].contiguous()
    depth[torch.from_numpy(rng.random((V, H, W)) < 0.05)] = 0
    color = torch.from_numpy(rng.integers(0, 256, (V, 3, H, W)).astype(np.float32))
    return torch.from_numpy(np.stack(proj).astype(np.float32)), depth, color


class TorchFusion:
    """the baseline: the reference's per-frame integrate restated with torch ops on the device -- one matrix product, masked gathers
    and masked scatters over the whole volume per frame"""

    def __init__(self, dims, voxel_size, origin, trunc_ratio, device):
        X, Y, Z = dims
        g = torch.arange(X * Y * Z, device=device)
        idx = torch.stack((g // (Y * Z), (g // Z) % Y, g % Z)).float()
        pts = idx * voxel_size + torch.tensor(origin, dtype=torch.float32, device=device).view(3, 1)
        self.pts = torch.cat((pts, torch.ones_like(pts[:1])))
        self.margin = voxel_size * trunc_ratio
        self.tsdf = torch.ones(X * Y * Z, device=device)
        self.weight = torch.zeros(X * Y * Z, device=device)
        self.color = torch.zeros(3, X * Y * Z, device=device)

    def reset(self):
        self.tsdf.fill_(1)
        self.weight.fill_(0)
        self.color.fill_(0)

    def integrate(self, P, depth, color):
        cam = P @ self.pts
        u = (cam[0] / cam[2]).round().long()
        v = (cam[1] / cam[2]).round().long()
        z = cam[2]
        h, w = depth.shape
        seen = (u >= 0) & (v >= 0) & (u < w) & (v < h) & (z > 0)
        keep = seen.clone()
        seen[keep] *= depth[v[keep], u[keep]] > 0
        sd = torch.clamp((z[seen] - depth[v[seen], u[seen]]) / self.margin, min=-1)
        inside = sd < 1
        keep = seen.clone()
        seen[keep] *= inside
        sd = sd[inside]
        empty = self.weight == 0
        self.tsdf[seen & empty] = sd[empty[seen]]
        near = seen.clone()
        near[seen] *= sd > -1
        add = ~empty & near
        self.tsdf[add] += sd[add[seen]]
        self.weight[near] += 1
        self.color[:, near] += color[:, v[near], u[near]]


def probe(dims, V, reps, warmup=3):
    dev = torch.device("cuda:0")
    proj, depth, color = (t.to(dev) for t in make_views(dims, V))
    lib = TSDFFusion(dims, VOXEL, (0.0, 0.0, 0.0), device=dev, color=True)
    base = TorchFusion(dims, VOXEL, (0.0, 0.0, 0.0), 3, dev)

    def single():
        for v in range(V):
            lib.integrate(proj[v], depth[v], color[v])

    def batched():
        lib.integrate(proj, depth, color)

    def baseline():
        for v in range(V):
            base.integrate(proj[v], depth[v], color[v])

    # the three agree (up to the baseline's device division) before anything is timed
    batched()
    want = (lib.tsdf_vol.clone(), lib.weight_vol.clone(), lib.color_vol.clone())
    lib.reset()
    single()
    same = all(torch.equal(a, b) for a, b in zip(want, (lib.tsdf_vol, lib.weight_vol, lib.color_vol)))
    baseline()
    differ = int(((base.tsdf != want[0]) | (base.weight != want[1]) | (base.color != want[2]).any(0)).sum())
    worst = float((base.tsdf - want[0]).abs().max())
    observed = int((want[1] > 0).sum())

    times = {"single": [], "batched": [], "torch": []}
    for r in range(warmup + reps):
        for name, fn in (("single", single), ("batched", batched), ("torch", baseline)):
            lib.reset()
            base.reset()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if r >= warmup:
                times[name].append(start.elapsed_time(stop) * 1e3 / V)                   # us per view
    n = math.prod(dims)
    row = dict(dims=list(dims), views=V, image=[H, W], reps=reps, observed_voxels=observed, single_equals_batched=same,
               torch_baseline_voxels_differing=differ, torch_baseline_largest_tsdf_difference=worst)
    for name, per_launch in (("single", 1), ("batched", V)):
        algo = 2 * 5 * 4 * n + 16 * H * W * per_launch
        med = statistics.median(times[name])
        row[f"{name}_algorithmic_bytes_per_launch"] = algo
        row[f"{name}_us_per_launch_at_8TBps"] = algo / HBM_BYTES_PER_S * 1e6
        row[f"{name}_share_of_8TBps"] = algo / HBM_BYTES_PER_S * 1e6 / (med * per_launch)
    for name, t in times.items():
        row[f"{name}_us_per_view_median"] = statistics.median(t)
        row[f"{name}_us_per_view_min"] = min(t)
    row["batched_no_slower_than_single"] = row["batched_us_per_view_median"] <= row["single_us_per_view_median"]
    row["single_no_slower_than_torch"] = row["single_us_per_view_median"] <= row["torch_us_per_view_median"]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", type=int, default=32)
    args = ap.parse_args()
    _lib.require_gpu()
    rows = [probe(d, args.views, args.reps) for d in SHAPES]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
