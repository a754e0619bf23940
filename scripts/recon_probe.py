"""Time of the TSDF head on the device (cnrma_amd.recon / csrc/recon.hip): python scripts/recon_probe.py [--out FILE.json] [--reps R]
[--trace DTYPE]

The three-scale head at the S shape -- decoder features of 128 / 64 / 32 channels on 48x48x20 -> 96x96x40 -> 192x192x80, B = 1,
label smoothing 1.05, thresholds 0.99 -- in fp32 and in bf16, two forms timed in the same run, alternating within every repetition,
each window closed by HIP events:
  device   AtlasTSDFHead(impl="device"): one forward launch per scale (+ two loss launches, + two backward launches)
  torch    the BASELINE: AtlasTSDFHead(impl="torch"), the module as it was before the device path existed -- conv3d, tanh,
           interpolate, where, boolean-index compaction and a host read per loss.  Never the code under test.
and two windows each:
  forward  no targets, no gradients (inference: what forward_test runs)
  train    forward + the three losses + backward of their sum to the features and the decoder weights
The features are drawn so that the coarse scales saturate in places: the share of far voxels per scale is reported, since the
device forward reads C values only for near voxels.  Reports medians and minima (20 repetitions after 3 warm-ups by default), the
algorithmic bytes of the forward (near voxels x C x element size + one fp32 store per voxel + the parents) with their time at
8 TB/s, the largest difference between the two forms' outputs away from the threshold, and whether device <= torch held.

--trace DTYPE (fp32 or bf16) only runs the device train window `reps` times, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/recon_probe.py --trace bf16): the event windows hold launch latency too."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import projects.mvsdetection  # noqa: E402,F401
from cnrma_amd import _lib  # noqa: E402
from projects.mvsdetection.registry import build_head  # noqa: E402

CHANNELS = (128, 64, 32)
GRIDS = ((48, 48, 20), (96, 96, 40), (192, 192, 80))
KEYS = ("016", "008", "004")
LS, THR = 1.05, 0.99
HBM_BYTES_PER_S = 8e12
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def head(impl, dev):
    h = build_head(dict(type="AtlasTSDFHead", input_channels=list(CHANNELS)[::-1], n_scales=3, voxel_size=0.04, label_smoothing=LS,
                        sparse_threshold=[THR] * 3, impl=impl)).to(dev)
    gen = torch.Generator().manual_seed(1)
    for dec, c in zip(h.decoders, CHANNELS):
        dec.weight.data.copy_((torch.randn(c, generator=gen) * 1.5 / c ** 0.5).reshape(dec.weight.shape))
    return h


def inputs(dtype, dev):
    gen = torch.Generator(device=dev).manual_seed(2)
    xs = [torch.randn(1, c, *g, generator=gen, device=dev).to(dtype) for c, g in zip(CHANNELS, GRIDS)]
    targets = {}
    for k, g in zip(KEYS, GRIDS):
        t = torch.rand(1, 1, *g, generator=gen, device=dev) * 2 - 1
        t[torch.rand(1, 1, *g, generator=gen, device=dev) < 0.2] = 1.0
        t[:, :, : g[0] // 4] = 1.0
        targets["tsdf_gt_" + k] = t
    return xs, targets


def windows(h, xs, targets):
    def forward():
        with torch.no_grad():
            return h(xs)[0]

    def train():
        leaves = [x.detach().requires_grad_(True) for x in xs]
        for p in h.parameters():
            p.grad = None
        out, losses = h(leaves, targets)
        sum(losses.values()).backward()
        return out
    return {"forward": forward, "train": train}


def probe(name, reps, warmup=3):
    dev = torch.device("cuda:0")
    dtype = DTYPES[name]
    xs, targets = inputs(dtype, dev)
    forms = {"device": windows(head("device", dev), xs, targets), "torch": windows(head("torch", dev), xs, targets)}
    out_d, out_t = forms["device"]["forward"](), forms["torch"]["forward"]()
    far, worst, flipped = [0.0], [], []
    for i, k in enumerate(KEYS):
        a, b = out_d["scene_tsdf_" + k], out_t["scene_tsdf_" + k]
        keep = torch.ones_like(a, dtype=torch.bool)
        if i:
            for parent in (out_d["scene_tsdf_" + KEYS[i - 1]], out_t["scene_tsdf_" + KEYS[i - 1]]):
                up = parent.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
                keep &= (up.abs() - THR).abs() > 1e-4
            far.append(float((~(up.abs() < THR)).float().mean()))
        worst.append(float((a - b)[keep].abs().max()))
        flipped.append(int((~keep).sum()))
    times = {(form, win): [] for form in forms for win in ("forward", "train")}
    for r in range(warmup + reps):
        for win in ("forward", "train"):
            for form in ("device", "torch"):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                forms[form][win]()
                stop.record()
                stop.synchronize()
                if r >= warmup:
                    times[(form, win)].append(start.elapsed_time(stop) * 1e3)              # us
    size = dtype.itemsize
    algo = sum(int(round((1 - f) * g[0] * g[1] * g[2])) * c * size + 4 * g[0] * g[1] * g[2] + (g[0] * g[1] * g[2] // 2 if i else 0)
               for i, (f, c, g) in enumerate(zip(far, CHANNELS, GRIDS)))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = dict(dtype=name, channels=list(CHANNELS), grids=[list(g) for g in GRIDS], reps=reps, far_share=far,
               largest_output_difference=worst, voxels_within_1e4_of_threshold_excluded=flipped,
               forward_algorithmic_bytes=algo, forward_us_at_8TBps=algo / HBM_BYTES_PER_S * 1e6)
    for (form, win), v in times.items():
        row[f"{form}_{win}_us_median"] = med[(form, win)]
        row[f"{form}_{win}_us_min"] = min(v)
    row["device_forward_share_of_8TBps"] = row["forward_us_at_8TBps"] / med[("device", "forward")]
    row["device_no_slower_forward"] = med[("device", "forward")] <= med[("torch", "forward")]
    row["device_no_slower_train"] = med[("device", "train")] <= med[("torch", "train")]
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", type=str, default=None, choices=sorted(DTYPES))
    args = ap.parse_args()
    _lib.require_gpu()
    if args.trace is not None:
        dev = torch.device("cuda:0")
        xs, targets = inputs(DTYPES[args.trace], dev)
        train = windows(head("device", dev), xs, targets)["train"]
        for _ in range(args.reps):
            train()
        torch.cuda.synchronize()
        sys.exit(0)
    rows = []
    for name in DTYPES:
        rows.append(probe(name, args.reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
