"""A/B of the march kernels (per-step sigmoid vs table-driven, free-space skipping off / on) at a workload shape: HIP-event
times (table builds included), interleaved; counts / sums / kept-sample records compared bit for bit.

    python scripts/march_ab.py NS [name=path/to/libcnrma_hip.so ...]

Every further library (another build of csrc/: the parent commit's, or this one with -DCNRMA_SKIP_JMIN=2) runs "table + free-space
skip" through the same buffers, in turn with this build's modes: one warm-up call each, then six rounds of one call each; the
series, their medians and spreads are printed."""
import ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cnrma_amd import _lib, rma, synth
wl = sys.argv[1] if len(sys.argv) > 1 else "NS"
ROUNDS = 6
dev = torch.device("cuda:0")
V, C, H, W, dims, stride = synth.SHAPES[wl]
sc = synth.make_scene((V, 8, H, W, dims, stride), seed=0, boxes=3)
feat = rma.to_nhwc(sc["features"][:, 0].to(dev))
pinv = rma.projection_inverse(sc["projection"][:, 0], stride).to(dev)
tsdf = sc["tsdf"][0, 0].to(dev)
m = rma._March(feat, pinv, tsdf, dims, 0.04, (0, 0, 0), 300, 0.05, "neus", 0)


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("cnrma_rma_skip_table_bytes", "cnrma_rma_march_tables_f32", "cnrma_rma_neus_march_f32", "cnrma_abi_version"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert lib.cnrma_abi_version() == _lib.ABI_VERSION
    return lib


this = _lib.load()
MODES = {"per-step sigmoid": (False, False, this), "table": (True, False, this), "table + free-space skip": (True, True, this)}
for arg in sys.argv[2:]:
    name, path = arg.split("=", 1)
    MODES[f"table + free-space skip [{name}]"] = (True, True, bind(path))
skips = {}          # one skip buffer per library: their sizes differ
res = {}
for rep in range(ROUNDS + 1):
    for name, (table, skip, lib) in MODES.items():
        rma.SIGMOID_TABLE, rma.MARCH_SKIP = table, skip
        _lib._libs[False] = lib                       # march() sizes the skip buffer and launches through this library
        m._skip = skips.get(id(lib))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = m.march(); b.record(); torch.cuda.synchronize()
        skips[id(lib)] = m._skip
        _lib._libs[False] = this
        if rep > 0:                                   # round 0 warms up (allocations, code objects)
            res.setdefault(name, []).append(a.elapsed_time(b))
        res[("out", name)] = out
for name in MODES:
    s = res[name]
    print(wl, f"{name:40s} ms:", [round(x, 3) for x in s], "median", round(statistics.median(s), 3), "spread",
          round(max(s) - min(s), 3))
c0, w0, k0, _ = res[("out", "per-step sigmoid")]
for name in list(MODES)[1:]:
    c1, w1, k1, _ = res[("out", name)]
    live = torch.arange(k0.shape[1], device=dev)[None, :] < c0[:, None].clamp(max=k0.shape[1])
    print(name, ": counts equal", torch.equal(c0, c1), "wsum equal", torch.equal(w0, w1), "records equal", bool((k0[live] == k1[live]).all()),
          "rays", c0.numel(), "kept", int(c0.sum()))
nb = 1
for d in dims:
    nb *= -(-d // 4)
head = skips[id(this)][:nb]
print("capped radii (blocks of 4^3 voxels):", {int(v): int((head == v).sum()) for v in (0, 4, 8, 12, 16)})
far_at = ((nb + 255) & ~255) + ((4 * nb + 255) & ~255)       # include/cnrma.h: layout of the skip buffer
far = skips[id(this)][far_at:far_at + nb]
print("far radii:", {int(v): int(c) for v, c in zip(*torch.unique(far, return_counts=True))})
