"""dense unprojection on 16-bit feature maps against the fp32 kernel at a workload shape: HIP-event times and bit equality.

    python scripts/dense_half_ab.py NS --rounds=6
    python scripts/dense_half_ab.py S --rounds=6

Maps are drawn in fp32 on the device (channels-last in memory) and cast to fp16 and to bf16.  Timed, one call of each in turn
per round after one warm-up call of each (clock and temperature drift hits all alike):

    f32            the fp32 kernel on the fp16 maps widened with .float() beforehand -- the kernel as it was, the baseline
    cast+f32       maps.float() + the fp32 kernel: what a user with 16-bit maps paid before (cast pass + a fp32 copy)
    fp16, bf16     the 16-bit kernel of the product library on the maps as they lie
    fp16/4 ...     C % 64 == 0 only: both forms of the 16-bit kernel (4 | 8 lanes per voxel) through the experiments library

`same`: bit equality of volume and count with the fp32 kernel's result on the same maps widened (each 16-bit type against its own).
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnrma_amd import rma, synth

rounds = 6
for a in [a for a in sys.argv if a.startswith("--rounds=")]:
    rounds = int(a.split("=")[1])
    sys.argv.remove(a)
wl = sys.argv[1] if len(sys.argv) > 1 else "NS"
dev = torch.device("cuda:0")
if "," in wl:                       # custom shape V,C,H,W,X,Y,Z,stride
    n = [int(x) for x in wl.split(",")]
    shape = (n[0], n[1], n[2], n[3], (n[4], n[5], n[6]), n[7])
else:
    shape = synth.SHAPES[wl]
V, C, H, W, dims, stride = shape
sc = synth.make_scene(shape, seed=0, device=dev, channels_last=True)
f32 = rma.to_nhwc(sc["features"][:, 0])
del sc["features"]
maps = {"fp16": f32.to(torch.float16), "bf16": f32.to(torch.bfloat16)}
del f32
wide = maps["fp16"].float()
proj = rma.scale_projection(sc["projection"][:, 0], stride).to(dev)


def kernel(feat):
    return rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj)


def config(name):
    """-> (tuning switches, callable)"""
    if name == "f32":
        return {}, lambda: kernel(wide)
    if name == "cast+f32":
        return {}, lambda: kernel(maps["fp16"].float())
    kind, _, lanes = name.partition("/")
    return (dict(lpv=int(lanes)) if lanes else {}), lambda: kernel(maps[kind])


def one_call(name):
    tune, fn = config(name)
    rma.dense_tuning(**tune)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); vol, cnt = fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), vol, cnt


names = ["f32", "cast+f32", "fp16", "bf16"]
if C % 64 == 0:
    names += ["fp16/4", "fp16/8", "bf16/4", "bf16/8"]
refs = {}
for kind in ("fp16", "bf16"):                             # the fp32 kernel on each type's maps widened: what `same` compares with
    vol, cnt = kernel(maps[kind].float())
    refs[kind] = (vol, cnt)
torch.cuda.synchronize()
same, series = {}, {s: [] for s in names}
try:
    for s in names:                                       # warm-up + bit equality
        _, vol, cnt = one_call(s)
        ref = refs["bf16" if s.startswith("bf16") else "fp16"]
        same[s] = torch.equal(vol, ref[0]) and torch.equal(cnt, ref[1])
        del vol, cnt
    del refs, ref
    for r in range(rounds):
        for s in names:
            t, vol, cnt = one_call(s)
            series[s].append(t)
            del vol, cnt
finally:
    rma.dense_tuning()
for s in names:
    ts = sorted(series[s])
    print(wl, s, "ms", [round(t, 3) for t in series[s]], "median", round(ts[len(ts) // 2], 3), "min", round(ts[0], 3),
          "max", round(ts[-1], 3), "same", same[s], flush=True)
