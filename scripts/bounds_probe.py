"""Time of the fusion-volume bounds (cnrma_amd.fusion.scene_bounds / csrc/bounds.hip): python scripts/bounds_probe.py [--out FILE.json]
[--reps R] [--views V] [--kernels-only]

Two ways to find the quantiles of the back-projected depth pixels of the same V posed depth maps, timed in the same run, alternating
within every repetition, each window a wall clock around a synchronised call (the baseline ends on the host):
  device    scene_bounds: V host inverses, four histogram passes over the depth maps (no cloud), one read of 80 bytes, numpy's
            interpolation on the host
  torch     the BASELINE: the reference's own form (generate_tsdf.py:82-101) restated in torch and numpy on the same machine -- per
            frame the mask, the inverse and the back-projection on the device, then the concatenation, the finite filter,
            .cpu().numpy() and two np.quantile.  Never the code under test.
Reports the median and minimum of each over R repetitions after 3 warm-ups, the device path's kernel time from HIP events around
cnrma_prep_depth_bounds_f32 alone, the algorithmic bytes (passes x 4 V H W: every pass reads each depth pixel once) and the share of
8 TB/s they reach in that kernel time, whether the expectation holds (device no slower than the baseline), and how far the baseline's
quantiles lie from the library's (the baseline multiplies and inverts on the device, so its last bits differ; the pinned behaviour is
the reference on the CPU).  --kernels-only launches cnrma_prep_depth_bounds_f32 alone (for a kernel trace taken in a run of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import _lib  # noqa: E402
from cnrma_amd.fusion import quantile_finish, scene_bounds  # noqa: E402

SHAPES = ((480, 640), (192, 256))
VOXEL, MAX_DEPTH, VOL_PRCNT, VOL_MARGIN, PASSES = 0.04, 3.0, 0.995, 1.5, 4
HBM_BYTES_PER_S = 8e12


def make_views(V, H, W, seed=0):
    """cameras on a ring inside a 7.7 x 7.7 x 3.2 m room looking across it, depth 0.5 - 4.5 m in smooth patches with 5 % holes"""
    rng = np.random.default_rng(seed)
    ext = np.array([7.68, 7.68, 3.2])
    centre, focal = 0.5 * ext, 577.0 * W / 640
    proj = []
    for a in 2 * np.pi * np.arange(V) / V:
        eye = centre + [0.3 * ext[0] * np.cos(a), 0.3 * ext[1] * np.sin(a), 0.1 * ext[2]]
        target = centre - [0.3 * ext[0] * np.cos(a), 0.3 * ext[1] * np.sin(a), 0.1 * ext[2]]
        f = (target - eye) / np.linalg.norm(target - eye)
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        R = np.stack((r, np.cross(f, r), f))
        K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])
        proj.append(K @ np.concatenate((R, (-R @ eye)[:, None]), axis=1))
    coarse = torch.from_numpy(rng.uniform(0.5, 4.5, (V, 1, 15, 20)).astype(np.float32))
    depth = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[:, 0].contiguous()
    depth[torch.from_numpy(rng.random((V, H, W), dtype=np.float32) < 0.05)] = 0
    return torch.from_numpy(np.stack(proj).astype(np.float32)), depth


def torch_baseline(proj, depth):
    """the reference's lines with torch ops on the device and numpy on the host -> (low, high) quantiles, the number of points"""
    pts = []
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=depth.device)
    for v in range(depth.shape[0]):
        d = depth[v].clone()
        d[d > MAX_DEPTH] = 0
        rows, cols = torch.meshgrid(torch.arange(d.shape[0], device=d.device, dtype=d.dtype),
                                    torch.arange(d.shape[1], device=d.device, dtype=d.dtype), indexing="ij")
        pixel = torch.stack((cols, rows, torch.ones_like(cols), 1 / d))
        world = torch.cat((proj[v], bottom)).inverse() @ pixel.view(4, -1)
        pts.append((world[:3] / world[3:]).T)
    pts = torch.cat(pts)
    pts = pts[torch.isfinite(pts[:, 0])].cpu().numpy()
    return np.quantile(pts, 1 - VOL_PRCNT, axis=0), np.quantile(pts, VOL_PRCNT, axis=0), len(pts)


def probe(V, H, W, reps, warmup=3, kernels_only=False):
    dev = torch.device("cuda:0")
    proj, depth = make_views(V, H, W)
    depth_dev, proj_dev = depth.to(dev), proj.to(dev)

    def device_path():
        return scene_bounds(proj, depth_dev, VOXEL, MAX_DEPTH, VOL_PRCNT, VOL_MARGIN, device=dev)

    # the kernels alone, between HIP events: the inverses and the buffers are made beforehand
    pinv = torch.stack([torch.inverse(torch.cat((P, torch.tensor([[0.0, 0.0, 0.0, 1.0]])))) for P in proj]).to(dev)
    nbytes = _lib.load_prep().cnrma_prep_bounds_workspace_bytes()
    ws, out = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.zeros(10, dtype=torch.int64, device=dev)

    def kernels():
        _lib.call_prep("cnrma_prep_depth_bounds_f32", _lib.ptr(pinv), _lib.ptr(depth_dev), V, H, W, MAX_DEPTH, 1 - VOL_PRCNT, VOL_PRCNT,
                       _lib.ptr(ws), nbytes, out.data_ptr() + 32, _lib.ptr(out), _lib.stream())

    if kernels_only:
        for _ in range(warmup + reps):
            kernels()
        torch.cuda.synchronize()
        return dict(views=V, image=[H, W], launches=warmup + reps)
    origin, dim = device_path()
    low, high, n = torch_baseline(proj_dev, depth_dev)
    kernels()
    got = out.cpu()
    values = got[4:].view(torch.float32).numpy().reshape(2, 3, 2)
    own = [quantile_finish(values[i, :, 0], values[i, :, 1], int(got[0]), q, got[1:4].numpy()) for i, q in enumerate((1 - VOL_PRCNT, VOL_PRCNT))]
    apart = float(max(np.abs(own[0] - low).max(), np.abs(own[1] - high).max()))

    wall = {"device": [], "torch": []}
    kernel_ms = []
    for r in range(warmup + reps):
        for name, fn in (("device", device_path), ("torch", lambda: torch_baseline(proj_dev, depth_dev))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        kernels()
        stop.record()
        stop.synchronize()
        if r >= warmup:
            kernel_ms.append(start.elapsed_time(stop))
    algo = PASSES * 4 * V * H * W
    row = dict(views=V, image=[H, W], pixels=V * H * W, kept=int(got[0]), baseline_kept=n, reps=reps, passes=PASSES,
               origin=origin.tolist(), voxel_dim=dim, baseline_quantiles_largest_difference=apart,
               algorithmic_bytes=algo, kernels_ms_median=statistics.median(kernel_ms), kernels_ms_min=min(kernel_ms),
               kernels_ms_at_8TBps=algo / HBM_BYTES_PER_S * 1e3,
               kernels_share_of_8TBps=algo / HBM_BYTES_PER_S * 1e3 / statistics.median(kernel_ms))
    for name, t in wall.items():
        row[f"{name}_ms_median"] = statistics.median(t)
        row[f"{name}_ms_min"] = min(t)
    row["baseline_over_device"] = row["torch_ms_median"] / row["device_ms_median"]
    row["device_no_slower_than_baseline"] = row["device_ms_median"] <= row["torch_ms_median"]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    _lib.require_gpu()
    rows = [probe(args.views, H, W, args.reps, kernels_only=args.kernels_only) for H, W in SHAPES[:1 if args.kernels_only else None]]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
