"""Time of the device TSDF resampling (cnrma_amd.resample / csrc/resample.hip): python scripts/resample_probe.py [--out FILE.json]
[--reps R] [--trace-level L]

The three ground-truth levels of a training sample -- a 230x210x90 scene at 4 cm into 192x192x80, and the same at 8 and 16 cm --
under the identity, a rotation about z and an oblique rotation (the last two about the volumes' centres), nine points.  Three
forms on the device, timed in the same run, alternating within every repetition, each window closed by HIP events:
  kernel   cnrma_amd.resample.resample_tsdf: staging of the origins and the transform, the output's allocation, one gather kernel
  entry    cnrma_tsdf_resample_f32 alone, everything staged beforehand: the kernel without the wrapper (for the share of 8 TB/s)
  torch    the BASELINE: the existing TSDF.transform on device tensors -- torch's own index grid, matrix product, two grid_sample
           passes and two masked overwrites.  Never the code under test.
and beside them the same TSDF.transform on the CPU (wall clock, fewer repetitions), which is what the loading pipeline runs today.
Reports the medians (20 repetitions after 3 warm-ups by default), the algorithmic bytes 4 X Y Z + 4 nx ny nz, their time at
8 TB/s and the share of it reached, the share of output voxels that are exactly +1, how many voxels of the baseline differ from the kernel's
result (a device's grid_sample and matrix product need not round like the pinned CPU path), and whether the expectation holds:
kernel <= torch at the point.

--trace-level L (0, 1, 2) only launches the entry form of that level under the rotation about z, `reps` times, for a kernel trace
taken in a run of its own (rocprofv3 --kernel-trace --stats -- python scripts/resample_probe.py --trace-level 0): the event windows
above hold a launch's latency, which at these sizes is most of them."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import _lib, synth  # noqa: E402
from cnrma_amd._lib import call, ptr, stream  # noqa: E402
from cnrma_amd.resample import resample_tsdf  # noqa: E402
from projects.mvsdetection.datasets.tsdf import TSDF  # noqa: E402

LEVELS = (((230, 210, 90), (192, 192, 80), 0.04), ((115, 105, 45), (96, 96, 40), 0.08), ((57, 52, 22), (48, 48, 20), 0.16))
HBM_BYTES_PER_S = 8e12
CPU_REPS, CPU_WARMUP = 5, 1


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def transforms(src_dim, dst_dim, vs):
    """identity; rotations about z and about (1, 1, 1) that map the centre of the new volume onto the centre of the old one"""
    out = {"identity": torch.eye(4)}
    sc, dc = 0.5 * vs * np.asarray(src_dim), 0.5 * vs * np.asarray(dst_dim)
    for name, R in (("rotation_z", rotation((0, 0, 1), 0.6)), ("oblique", rotation((1, 1, 1), 0.5))):
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = sc - R @ dc
        out[name] = torch.from_numpy(T.astype(np.float32))
    return out


def probe(src_dim, dst_dim, vs, name, T, reps, warmup=3):
    dev = torch.device("cuda:0")
    vol = synth.room_tsdf(src_dim, voxel_size=vs, boxes=4, seed=3)[0, 0].contiguous()
    host = TSDF(vs, torch.zeros(1, 3), vol)
    src = TSDF(vs, torch.zeros(1, 3, device=dev), vol.to(dev))
    lazy = TSDF(vs, torch.zeros(1, 3), src.tsdf_vol)         # as the detector resolves a deferred volume: origins and transform on the host
    Td = T.to(dev)

    def kernel():
        return resample_tsdf(lazy, T, dst_dim, (0, 0, 0)).tsdf_vol

    staged = torch.cat((torch.zeros(3), T[:3].reshape(12), torch.zeros(3))).to(dev)
    out = torch.empty(dst_dim, device=dev)

    def entry():
        call("cnrma_tsdf_resample_f32", ptr(src.tsdf_vol), *src_dim, ptr(staged[:3]), vs, ptr(staged[3:15]), ptr(staged[15:]), *dst_dim,
             ptr(out), stream())
        return out

    def baseline():
        return src.transform(Td, list(dst_dim), [0, 0, 0]).tsdf_vol

    got, base = kernel(), baseline()
    assert torch.equal(entry(), got)
    differ = int((got != base).sum())
    worst = float((got - base).abs().max())
    border = float((got == 1).float().mean())
    times = {"kernel": [], "entry": [], "torch": []}
    for r in range(warmup + reps):
        for form, fn in (("kernel", kernel), ("entry", entry), ("torch", baseline)):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if r >= warmup:
                times[form].append(start.elapsed_time(stop) * 1e3)                     # us
    cpu = []
    for r in range(CPU_WARMUP + CPU_REPS):
        t0 = time.perf_counter()
        ref = host.transform(T, list(dst_dim), [0, 0, 0]).tsdf_vol
        if r >= CPU_WARMUP:
            cpu.append((time.perf_counter() - t0) * 1e6)
    algo = 4 * math.prod(src_dim) + 4 * math.prod(dst_dim)
    k, e, t = (statistics.median(times[form]) for form in ("kernel", "entry", "torch"))
    return dict(src_dim=list(src_dim), dst_dim=list(dst_dim), voxel_size=vs, transform=name, reps=reps,
                kernel_us_median=k, kernel_us_min=min(times["kernel"]), entry_us_median=e, entry_us_min=min(times["entry"]),
                torch_device_us_median=t, torch_device_us_min=min(times["torch"]),
                host_cpu_us_median=statistics.median(cpu), host_cpu_threads=torch.get_num_threads(), host_cpu_reps=CPU_REPS,
                algorithmic_bytes=algo, us_at_8TBps=algo / HBM_BYTES_PER_S * 1e6, kernel_share_of_8TBps=algo / HBM_BYTES_PER_S * 1e6 / k,
                entry_share_of_8TBps=algo / HBM_BYTES_PER_S * 1e6 / e,
                share_of_ones_in_output=border, kernel_voxels_differing_from_host_cpu=int((got.cpu() != ref).sum()),
                torch_device_voxels_differing_from_kernel=differ, torch_device_largest_difference=worst,
                kernel_no_slower_than_torch_device=k <= t)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-level", type=int, default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    if args.trace_level is not None:
        src_dim, dst_dim, vs = LEVELS[args.trace_level]
        dev = torch.device("cuda:0")
        vol = synth.room_tsdf(src_dim, voxel_size=vs, boxes=4, seed=3)[0, 0].contiguous().to(dev)
        staged = torch.cat((torch.zeros(3), transforms(src_dim, dst_dim, vs)["rotation_z"][:3].reshape(12), torch.zeros(3))).to(dev)
        out = torch.empty(dst_dim, device=dev)
        for _ in range(args.reps):
            call("cnrma_tsdf_resample_f32", ptr(vol), *src_dim, ptr(staged[:3]), vs, ptr(staged[3:15]), ptr(staged[15:]), *dst_dim,
                 ptr(out), stream())
        torch.cuda.synchronize()
        sys.exit(0)
    rows = []
    for src_dim, dst_dim, vs in LEVELS:
        for name, T in transforms(src_dim, dst_dim, vs).items():
            rows.append(probe(src_dim, dst_dim, vs, name, T, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
