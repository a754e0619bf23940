"""Time of the 3D U-Net with its 3x3x3 convolutions on the device (cnrma_amd.unet / csrc/unet.hip):
python scripts/unet_probe.py [--out FILE.json] [--seconds S] [--shapes 192x192x80,256x256x96] [--trace SHAPE] [--joints]

1. The eval forward of the shipped network (_builders.backbone_3d_cfg(): channels 32 / 64 / 128 / 256, layers_down [1, 2, 3, 4],
   layers_up [3, 2, 1]) at B = 1, two forms timed in the same run, alternating within every repetition, each window closed by HIP
   events, both warmed first, each over at least `seconds` of work:
     torch    the BASELINE: AtlasBackbone3D(impl="torch"), the module as it was before the device path existed (MIOpen).
     device   AtlasBackbone3D(impl="device").
   Reports medians, minima and maxima, the largest difference between the two forms' outputs (helpers' elementwise criterion), and
   the device forward's split into its 3x3x3 launches (each call closed by its own events, in repetitions of their own) and the
   rest (the torch glue: 1x1x1 convolutions, up-sampling, skip arithmetic).
2. Per level, one stride-1 convolution C -> C with folded BatchNorm and ReLU at that level's grid: its time, the FLOP/s from
   2 * 27 * Cin * Cout * voxels, as a share of one third of the measured fp16 matrix ceiling (f16x3 spends three products per
   product; 2.44 PFLOP/s, scripts/mfma_peak.hip), the bytes bound (x read once, y written once, at 8 TB/s) and which of the two
   bounds is the larger.
3. Registers, LDS and occupancy of every unet_conv3_kernel instantiation from csrc/unet.resources.txt, when the build left it.

--joints runs the decoder-joint comparison instead (cnrma_amd.unet.join / csrc/unet_join.hip), by the same rules: the eval forward with
impl="device" in two forms, joints="torch" (the BASELINE: the joints as torch ops, the module before the fused joints existed) and
joints="device", both warmed, alternating within every repetition, each over at least `seconds` of work, HIP-event windows, median
[min, max]; for the shipped network (cond_proj=False) and with cond_proj=True.  Then every joint of the decoder alone at its grid --
the three launches of one unet.join call inside one event window -- beside its bytes bound: the skip read once, the joined volume
written once and the coarse state read once, at the 6.3 TB/s a streaming kernel achieves; the scratch of the coarse product (written and
read back through the cache) is listed beside it.  Last, observed_mask with its bound beside one read of the input.

--trace SHAPE only runs the device forward for `seconds`, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python scripts/unet_probe.py --trace 192x192x80): the event windows hold launch latency too."""
import argparse
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import projects.mvsdetection  # noqa: E402,F401
from cnrma_amd import _lib, unet  # noqa: E402
from projects.configs.mvsdetection._builders import backbone_3d_cfg  # noqa: E402
from projects.mvsdetection.registry import build_backbone  # noqa: E402

MFMA_F16_FLOPS, HBM_BYTES_PER_S = 2.44e15, 8e12


def network(impl, dev, **over):
    torch.manual_seed(1)
    net = build_backbone(dict(backbone_3d_cfg(), impl=impl, **over)).eval()
    gen = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for m in net.modules():                                    # non-trivial statistics; residual branches switched on
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.copy_(1 + 0.1 * torch.randn(m.weight.shape, generator=gen))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=gen))
                m.running_var.copy_(0.5 + 0.5 * torch.randn(m.bias.shape, generator=gen).abs())
    return net.to(dev).requires_grad_(False)


def elementwise_error(a, b):
    err = (a.double() - b.double()).abs()
    return float(torch.minimum(err, err / b.double().abs().clamp_min(1e-300)).max())


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop), out                             # ms


def spread(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), reps=len(v))


def conv3_flop(channels, layers_down, layers_up, dims):
    total, vox = 0, dims[0] * dims[1] * dims[2]
    for i, c in enumerate(channels):
        if i:
            vox = ((dims[0] - 1) // 2 ** i + 1) * ((dims[1] - 1) // 2 ** i + 1) * ((dims[2] - 1) // 2 ** i + 1)
            total += 2 * 27 * channels[i - 1] * c * vox
        blocks = layers_down[i] + (layers_up[len(channels) - 2 - i] if i < len(channels) - 1 else 0)
        total += 2 * blocks * 2 * 27 * c * c * vox
    return total


def probe_network(dims, seconds, dev):
    x = torch.randn(1, 32, *dims, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    x[:, :, : dims[0] // 4] = 0
    nets = {"torch": network("torch", dev), "device": network("device", dev)}
    outs = {}
    with torch.no_grad():
        for form, net in nets.items():                               # warm both: MIOpen's choices, the library, the weight images
            t0 = time.time()
            for _ in range(2):
                outs[form] = net(x)
            torch.cuda.synchronize()
            print(f"  warmed {form} at {dims} in {time.time() - t0:.1f} s", flush=True)
        diff = [elementwise_error(a, b) for a, b in zip(outs["device"], outs["torch"])]
        outs.clear()
        times, total = {"torch": [], "device": []}, {"torch": 0.0, "device": 0.0}
        while min(total.values()) < seconds * 1e3 or len(times["torch"]) < 5:
            for form in ("torch", "device"):
                ms, _ = timed(lambda: nets[form](x))
                times[form].append(ms)
                total[form] += ms
        # the split: every conv3 call of the device forward closed by its own events
        calls, plain = [], unet.conv3

        def conv3_timed(*a, **k):
            ms, out = timed(lambda: plain(*a, **k))
            calls[-1].append(ms)
            return out
        unet.conv3 = conv3_timed
        try:
            for _ in range(3):
                calls.append([])
                nets["device"](x)
        finally:
            unet.conv3 = plain
    conv_ms = statistics.median(sum(c) for c in calls)
    cfg = backbone_3d_cfg()
    flop = conv3_flop(cfg["channels"], cfg["layers_down"], cfg["layers_up"], dims)
    dev_ms = statistics.median(times["device"])
    return dict(dims=list(dims), torch=spread(times["torch"]), device=spread(times["device"]), conv3_launches=len(calls[0]),
                device_conv3_ms=conv_ms, device_rest_ms=dev_ms - conv_ms, conv3_flop=flop,
                device_conv3_share_of_ceiling=flop / (conv_ms * 1e-3) / (MFMA_F16_FLOPS / 3),
                output_difference_device_vs_torch=diff, device_faster=dev_ms < statistics.median(times["torch"]))


def probe_levels(dims, seconds, dev):
    rows = []
    for i, c in enumerate(backbone_3d_cfg()["channels"]):
        d = tuple((n - 1) // 2 ** i + 1 for n in dims)
        gen = torch.Generator(device=dev).manual_seed(10 + i)
        x = torch.randn(1, c, *d, generator=gen, device=dev)
        image = unet.prepare_conv3_weights(torch.randn(c, c, 3, 3, 3, generator=gen, device=dev) * (2 / (27 * c)) ** 0.5)
        scale, shift = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        bound = unet.absmax(x)
        run = lambda: unet.conv3(x, image, scale=scale, shift=shift, relu=True, bound=bound)
        for _ in range(3):
            run()
        times, total = [], 0.0
        while total < seconds * 250 or len(times) < 10:             # a quarter of the window per level
            ms, _ = timed(run)
            times.append(ms)
            total += ms
        vox = d[0] * d[1] * d[2]
        flop, nbytes = 2 * 27 * c * c * vox, 2 * 4 * c * vox
        med = statistics.median(times)
        mfma_ms, bytes_ms = flop / (MFMA_F16_FLOPS / 3) * 1e3, nbytes / HBM_BYTES_PER_S * 1e3
        rows.append(dict(level=i, channels=c, dims=list(d), **spread(times), flop=flop, flops_achieved=flop / (med * 1e-3),
                         share_of_third_of_mfma_ceiling=mfma_ms / med, mfma_bound_ms=mfma_ms, bytes=nbytes, bytes_bound_ms=bytes_ms,
                         larger_bound="matrix" if mfma_ms >= bytes_ms else "bytes"))
        print("  level", json.dumps(rows[-1]), flush=True)
    return rows


STREAM_BYTES_PER_S = 6.3e12         # what a streaming kernel achieves on this part


def probe_joints_network(dims, seconds, dev, cond):
    x = torch.randn(1, 32, *dims, generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    x[:, :, : dims[0] // 4] = 0
    nets = {form: network("device", dev, joints=form, cond_proj=cond) for form in ("torch", "device")}
    outs = {}
    with torch.no_grad():
        for form, net in nets.items():                               # warm both: the GEMM choices, the libraries, the weight images
            for _ in range(3):
                outs[form] = net(x)
            torch.cuda.synchronize()
        diff = [elementwise_error(a, b) for a, b in zip(outs["device"], outs["torch"])]
        outs.clear()
        times, total = {"torch": [], "device": []}, {"torch": 0.0, "device": 0.0}
        while min(total.values()) < seconds * 1e3 or len(times["torch"]) < 5:
            for form in ("torch", "device"):
                ms, _ = timed(lambda: nets[form](x))
                times[form].append(ms)
                total[form] += ms
    row = dict(dims=list(dims), cond_proj=cond, joints_torch=spread(times["torch"]), joints_device=spread(times["device"]),
               output_difference_device_vs_torch=diff)
    row["ranges_disjoint_device_faster"] = row["joints_device"]["max_ms"] < row["joints_torch"]["min_ms"]
    return row


def probe_joints_alone(dims, seconds, dev):
    rows, chans = [], backbone_3d_cfg()["channels"][::-1]
    level = lambda i: tuple((n - 1) // 2 ** i + 1 for n in dims)
    for j in range(1, len(chans)):
        cc, cf, lc, lf = chans[j - 1], chans[j], level(len(chans) - j), level(len(chans) - 1 - j)
        if tuple(2 * n for n in lc) != lf:
            rows.append(dict(joint=j - 1, coarse=list(lc), fine=list(lf), skipped="the fine grid is not twice the coarse one"))
            continue
        gen = torch.Generator(device=dev).manual_seed(20 + j)
        xc, e = torch.randn(1, cc, *lc, generator=gen, device=dev), torch.randn(1, cf, *lf, generator=gen, device=dev)
        w_up = torch.randn(cf, cc, generator=gen, device=dev) * (2 / cc) ** 0.5
        w_proj = torch.randn(cf, cf, generator=gen, device=dev) * (2 / cf) ** 0.5
        scale, shift = torch.ones(cf, device=dev), torch.zeros(cf, device=dev)
        step = 2 ** (len(chans) - 1 - j)
        observed = (torch.rand(1, *dims, generator=gen, device=dev) < 0.6).to(torch.uint8)
        out = torch.empty_like(e)
        scratch = torch.empty(_lib.load_unet_join().cnrma_unet_join_scratch_bytes(1, cc, cf, *lc), dtype=torch.uint8, device=dev)
        row = dict(joint=j - 1, channels=[cc, cf], coarse=list(lc), fine=list(lf), step=step)
        for name, obs in (("plain", None), ("masked", observed)):
            run = lambda: unet.join(xc, e, w_up, w_proj, scale, shift, observed=obs, step=step, out=out, scratch=scratch)
            for _ in range(3):
                run()
            times, total = [], 0.0
            while total < seconds * 125 or len(times) < 10:          # an eighth of the window per joint and form
                ms, _ = timed(run)
                times.append(ms)
                total += ms
            row[name] = spread(times)
        vf, vc = lf[0] * lf[1] * lf[2], lc[0] * lc[1] * lc[2]
        nbytes = dict(skip_read=4 * cf * vf, joined_written=4 * cf * vf, coarse_read=4 * cc * vc, scratch_written_and_read=2 * 4 * cf * vc)
        bound = (nbytes["skip_read"] + nbytes["joined_written"] + nbytes["coarse_read"]) / STREAM_BYTES_PER_S * 1e3
        row.update(bytes=nbytes, bytes_bound_ms=bound, plain_over_bound=row["plain"]["median_ms"] / bound,
                   flop=2 * cf * (cf * vf + cc * vc))
        rows.append(row)
        print("  joint", json.dumps(row), flush=True)
    return rows


def probe_observed(dims, seconds, dev):
    x = torch.randn(1, 32, *dims, generator=torch.Generator(device=dev).manual_seed(4), device=dev)
    forms = {"observed_mask_with_bound": lambda: unet.observed_mask(x, with_bound=True),
             "torch_mask_and_absmax": lambda: ((x != 0).any(1, keepdim=True).float(), unet.absmax(x))}
    times = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(3):
            fn()
    total = 0.0
    while total < seconds * 250 or len(times["observed_mask_with_bound"]) < 10:
        for k, fn in forms.items():
            ms, _ = timed(fn)
            times[k].append(ms)
        total += times["observed_mask_with_bound"][-1]
    return dict(dims=list(dims), bytes_read=x.numel() * 4, bytes_bound_ms=x.numel() * 4 / STREAM_BYTES_PER_S * 1e3,
                **{k: spread(v) for k, v in times.items()})


def resources(name="unet.resources.txt", kernels="unet_conv3_kernel"):
    path = os.path.join(ROOT, "cn-rma_amd", "csrc", name)
    if not os.path.exists(path):
        return None
    if kernels != "unet_conv3_kernel":
        rows, cur = [], None
        for line in open(path):
            if m := re.search(r"Function Name: \S*?(" + kernels + r"\w*?kernel)", line):
                cur = dict(kernel=m.group(1))
                rows.append(cur)
            elif "Function Name:" in line:
                cur = None
            elif cur is not None and (m := re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                                                      r"LDS Size \[bytes/block\]): (\d+)", line)):
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
        return rows
    rows, cur = [], None
    for line in open(path):
        if m := re.search(r"Function Name: (\S+)", line):
            cur = dict(kernel=m.group(1)) if "unet_conv3_kernel" in m.group(1) else None
            if cur is not None:
                t = re.search(r"unet_conv3_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", cur["kernel"])
                cur.update(kernel="unet_conv3_kernel<%s, %s, %s, %s>" % t.groups(), stride=int(t.group(1)), channel_tiles=int(t.group(3)))
                rows.append(cur)
        elif cur is not None and (m := re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                                                  r"LDS Size \[bytes/block\]): (\d+)", line)):
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--shapes", type=str, default="192x192x80,256x256x96")
    ap.add_argument("--trace", type=str, default=None)
    ap.add_argument("--joints", action="store_true")
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    parse = lambda s: tuple(int(n) for n in s.split("x"))
    if args.trace is not None:
        dims = parse(args.trace)
        net, x = network("device", dev), torch.randn(1, 32, *dims, device=dev)
        t0 = time.time()
        with torch.no_grad():
            while time.time() - t0 < args.seconds:
                net(x)
                torch.cuda.synchronize()
        sys.exit(0)
    if args.joints:
        result = dict(stream_bytes_per_s=STREAM_BYTES_PER_S, networks=[], joints=[], observed=[],
                      resources=resources("unet_join.resources.txt", "unetjoin_"))
        for shape in args.shapes.split(","):
            dims = parse(shape)
            for cond in (False, True):
                result["networks"].append(probe_joints_network(dims, args.seconds, dev, cond))
                print(json.dumps(result["networks"][-1]), flush=True)
            result["joints"].append(dict(dims=list(dims), rows=probe_joints_alone(dims, args.seconds, dev)))
            result["observed"].append(probe_observed(dims, args.seconds, dev))
            print(json.dumps(result["observed"][-1]), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(result, f, indent=1)
        sys.exit(0)
    result = dict(mfma_f16_flops=MFMA_F16_FLOPS, hbm_bytes_per_s=HBM_BYTES_PER_S, networks=[], levels=[], resources=resources())
    for shape in args.shapes.split(","):
        dims = parse(shape)
        result["networks"].append(probe_network(dims, args.seconds, dev))
        print(json.dumps(result["networks"][-1]), flush=True)
        result["levels"].append(dict(dims=list(dims), rows=probe_levels(dims, args.seconds, dev)))
        if args.out:                                                 # after every shape: a partial run leaves what it measured
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
