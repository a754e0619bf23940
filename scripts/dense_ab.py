"""dense unprojection kernel at a workload shape under different schedule switches (rma.dense_tuning): HIP-event times
and bit equality with the first configuration.

    python scripts/dense_ab.py NS variant=0 variant=1 variant=1,epi=1 variant=1,st=32,lockstep=1 ...
    python scripts/dense_ab.py NS --rounds=6 default zrun=0          (old against new lane mapping, alternating)

--rounds=N: after one warm-up call of every configuration, N rounds that time ONE call of each configuration in turn, so that
clock and temperature drift hits all of them alike; prints each configuration's series, its median and its spread.
"default" is the product library; any switch (zrun=0: the round-3 lane mapping with 4-byte stores; nt=1 | 2: non-temporal |
write-through volume stores) goes through the experiments library.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnrma_amd import rma, synth

rounds = 0
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
sc = synth.make_scene(shape, seed=0, device=dev)
feat = rma.to_nhwc(sc["features"][:, 0])
del sc["features"]
proj = rma.scale_projection(sc["projection"][:, 0], stride).to(dev)
ref = None


def parse(spec):
    return {} if spec == "default" else {k: int(v) for k, v in (kv.split("=") for kv in spec.split(","))}


def one_call(spec):
    rma.dense_tuning(**parse(spec))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); vol, cnt = rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), vol, cnt


if rounds:
    specs = sys.argv[2:] or ["default"]
    same, series = {}, {s: [] for s in specs}
    for s in specs:                                       # warm-up + bit equality with the first configuration
        _, vol, cnt = one_call(s)
        if ref is None:
            ref = (vol.clone(), cnt.clone())
        same[s] = torch.equal(vol, ref[0]) and torch.equal(cnt, ref[1])
        del vol, cnt
    for r in range(rounds):
        for s in specs:
            t, vol, cnt = one_call(s)
            series[s].append(t)
            del vol, cnt
    for s in specs:
        ts = sorted(series[s])
        print(wl, s, "ms", [round(t, 3) for t in series[s]], "median", round(ts[len(ts) // 2], 3), "min", round(ts[0], 3),
              "max", round(ts[-1], 3), "same", same[s], flush=True)
    rma.dense_tuning()
    sys.exit(0)

for spec in sys.argv[2:] or ["default"]:
    rma.dense_tuning(**parse(spec))
    ts = []
    for rep in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); vol, cnt = rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj); b.record()
        torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    if ref is None:
        ref = (vol.clone(), cnt.clone())
    print(wl, spec, "ms", [round(t, 3) for t in ts], "same", torch.equal(vol, ref[0]) and torch.equal(cnt, ref[1]), flush=True)
    del vol, cnt
rma.dense_tuning()
