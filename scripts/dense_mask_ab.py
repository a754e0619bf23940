"""dense unprojection kernel with and without the per-wave view masks, in one process on one library: HIP-event times (the
recording sweep is inside the masked time) and bit equality with the first configuration.

    python scripts/dense_mask_ab.py NS                                          (masked, unmasked; 6 rounds)
    python scripts/dense_mask_ab.py S --rounds=6 masked unmasked masked,st=32,zt=32 unmasked,st=32,zt=32

A configuration is "masked" (a workspace with room for the table) or "unmasked" (the 1024-byte workspace: every view walked),
optionally followed by schedule switches of the experiments library (rma.dense_tuning).  After one warm-up call of every
configuration, N rounds time ONE call of each in turn, so that clock and temperature drift hits all of them alike; prints each
configuration's series, median, min and max.  --warmup=N: N warm-up calls of every configuration (a fresh process needs more than
one before its first timed call is no outlier); the shape is a workload name or V,C,H,W,X,Y,Z,stride.  In a tree from before the masks (no rma.dense_workspace) only "unmasked" runs:
the same script then times the parent's kernel for comparison.
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnrma_amd import rma, synth

rounds, warmup = 6, 1
for a in [a for a in sys.argv if a.startswith("--rounds=") or a.startswith("--warmup=")]:
    if a.startswith("--rounds="):
        rounds = int(a.split("=")[1])
    else:
        warmup = int(a.split("=")[1])
    sys.argv.remove(a)
wl = sys.argv[1] if len(sys.argv) > 1 else "NS"
has_masks = hasattr(rma, "dense_workspace")
specs = sys.argv[2:] or (["masked", "unmasked"] if has_masks else ["unmasked"])
dev = torch.device("cuda:0")
shape = synth.SHAPES[wl] if "," not in wl else (lambda n: (n[0], n[1], n[2], n[3], (n[4], n[5], n[6]), n[7]))([int(x) for x in wl.split(",")])
V, C, H, W, dims, stride = shape
sc = synth.make_scene(shape, seed=0, device=dev)
feat = rma.to_nhwc(sc["features"][:, 0])
del sc["features"]
proj = rma.scale_projection(sc["projection"][:, 0], stride).to(dev)
ws = {"masked": rma.dense_workspace(dev, dims, V) if has_masks else None, "unmasked": torch.zeros(256, dtype=torch.int32, device=dev)}


def one_call(spec):
    mode, _, rest = spec.partition(",")
    assert mode in ws and (has_masks or mode == "unmasked"), spec
    rma.dense_tuning(**({k: int(v) for k, v in (kv.split("=") for kv in rest.split(","))} if rest else {}))
    kw = dict(workspace=ws[mode]) if has_masks else {}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); vol, cnt = rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj, **kw); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), vol, cnt


ref, same, series = None, {}, {s: [] for s in specs}
for s in specs * warmup:                              # warm-up + bit equality with the first configuration
    _, vol, cnt = one_call(s)
    if ref is None:
        ref = (vol.clone(), cnt.clone())
        print(wl, "checksum of", s, "count", int(cnt.sum()), "volume", float(vol.double().abs().sum()), flush=True)
    same[s] = torch.equal(vol, ref[0]) and torch.equal(cnt, ref[1])
    del vol, cnt
for r in range(rounds):
    for s in specs:
        t, vol, cnt = one_call(s)
        series[s].append(t)
        del vol, cnt
for s in specs:
    ts = sorted(series[s])
    if ts:
        print(wl, s, "ms", [round(t, 3) for t in series[s]], "median", round(ts[len(ts) // 2], 3), "min", round(ts[0], 3),
              "max", round(ts[-1], 3), "same", same[s], flush=True)
rma.dense_tuning()
