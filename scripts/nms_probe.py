"""Per-class 3D NMS: the class-by-class host path (postprocess.nms) against the device path (postprocess.nms_device), and a scene
graph with and without the NMS stage.

    python scripts/nms_probe.py --rounds=8

Blocks: the raw detections of one StaticScene replay of a synthetic S scene -- ScanNet head (18 classes, axis-aligned boxes) and
ARKit head (17 classes, rotated boxes), 4 levels x nms_pre 1000 = 4000 rows each.  The heads are untrained, so few of their
scores pass 0.01; `drawn` keeps the boxes of the block and replaces the scores with a seeded draw u^3 (four fifths of every
class are candidates: the load of a cluttered scene).  Per block and round, one after the other (drift hits all alike), each
timed with the host clock around a call that ends in a synchronise:

    host      postprocess.nms: per class nonzero, sort, mask launch, mask read-back, Python scan
    device    postprocess.nms_device: four launches, one read (the count)
    padded    postprocess.nms_device(padded=True): the four launches alone, no read (what a scene graph appends)

and `same`: torch.equal of the three outputs.  Reads: calls of _lib.read_ints inside one nms_device call; the padded form
additionally runs once with torch's sync debug mode set to "error".
Scene: S-shape StaticScene replays, a slot with nms=dict(score_thr=0.01, iou_thr=0.5) and one without, alternating; graph nodes
of both.  Medians over the rounds; min .. max beside them."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from cnrma_amd import _lib, pipeline, synth
from cnrma_amd import postprocess as PP

rounds = 8
for a in [a for a in sys.argv if a.startswith("--rounds=")]:
    rounds = int(a.split("=")[1])
rounds = max(rounds, 6)
wl = "S"
for a in [a for a in sys.argv[1:] if not a.startswith("--")]:
    wl = a                                                  # another synth shape (rehearsals)
dev = torch.device("cuda:0")
NMS = dict(score_thr=0.01, iou_thr=0.5)
V, C, H, W, dims, stride = synth.SHAPES[wl]
sc = synth.make_scene(wl, seed=0, boxes=3, device=dev)
feat, proj, tsdf = sc["features"][:, 0].to(dev), sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev)
cfg = pipeline.SceneConfig(dims, stride=stride, max_points=500000, sampler="device", sample_seed=0)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def line(name, xs):
    return f"{name:>8} {statistics.median(xs):9.3f} ms   ({min(xs):.3f} .. {max(xs):.3f})"


def raw_block(n_classes, n_reg):
    backbone, head = bench.build_model(C, dev, n_classes=n_classes, n_reg=n_reg)
    slot = pipeline.StaticScene(cfg, backbone, head, dev, dense=False)
    slot.build(feat, proj, tsdf)
    out = slot.run(feat, proj, tsdf)
    torch.cuda.synchronize()
    b, s, _ = pipeline.StaticScene.detections(out)
    return b.clone(), s.clone()


def compare(name, b, s):
    n, n_cls = s.shape
    cand = (s > NMS["score_thr"]).sum(0)
    print(f"\n{name}: {n} x {n_cls}, {b.shape[1]} columns; candidates per class min {int(cand.min())} / median "
          f"{int(cand.median())} / max {int(cand.max())}")
    bufs = PP.nms_device_buffers(n, n_cls, b.shape[1], dev)
    host = lambda: PP.nms(b, s, **NMS)
    device = lambda: PP.nms_device(b, s, out=bufs, **NMS)
    padded = lambda: PP.nms_device(b, s, padded=True, out=bufs, **NMS)
    exp, got = host(), device()                             # warm-up
    padded()
    same = all(torch.equal(g, e) for g, e in zip(got, exp))
    reads, orig = [0], _lib.read_ints
    def counting(t):
        reads[0] += 1
        return orig(t)
    _lib.read_ints = counting
    try:
        device()
    finally:
        _lib.read_ints = orig
    strict = "not checked"
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            padded()
            strict = "no synchronising call"
        finally:
            torch.cuda.set_sync_debug_mode("default")
    except Exception as e:                                   # noqa: BLE001 -- reported, not hidden
        strict = f"{type(e).__name__}: {e}"
    torch.cuda.synchronize()
    series = dict(host=[], device=[], padded=[])
    for _ in range(rounds):
        for key, fn in (("host", host), ("device", device), ("padded", padded)):
            series[key].append(wall(fn)[0])
    for key in series:
        print(line(key, series[key]))
    print(f"    kept {len(exp[0])}; same {same}; host reads in nms_device: {reads[0]}; padded under sync debug: {strict}")
    print(f"    host / device = {statistics.median(series['host']) / statistics.median(series['device']):.1f}x")


with torch.no_grad():
    print(f"nms_probe: shape {wl}, rounds {rounds}, device {torch.cuda.get_device_name(0)}")
    for name, n_classes, n_reg in (("ScanNet", 18, 6), ("ARKit", 17, 8)):
        b, s = raw_block(n_classes, n_reg)
        compare(f"{name} raw block", b, s)
        g = torch.Generator(device=dev).manual_seed(1)
        compare(f"{name} drawn scores", b, torch.rand(s.shape, generator=g, device=dev) ** 3)
        del b, s

    # ---- the scene graph with and without the stage
    backbone, head = bench.build_model(C, dev)
    plain = pipeline.StaticScene(cfg, backbone, head, dev)
    plain.build(feat, proj, tsdf)
    with_nms = pipeline.StaticScene(cfg, backbone, head, dev, nms=NMS)
    with_nms.build(feat, proj, tsdf, plan=plain.plan)
    REPS = 10

    def replay(slot):
        for _ in range(REPS):
            out = slot.run(feat, proj, tsdf)
        return out

    replay(plain), replay(with_nms)
    torch.cuda.synchronize()
    series = dict(plain=[], nms=[])
    for _ in range(rounds):
        series["plain"].append(wall(lambda: replay(plain))[0] / REPS)
        series["nms"].append(wall(lambda: replay(with_nms))[0] / REPS)
    out = with_nms.run(feat, proj, tsdf)
    k = len(pipeline.StaticScene.final_detections(out)[0])
    print(f"\nscene graph, shape {wl}, {REPS} replays per sample: rows {out['bboxes'].shape[0]}, final detections {k}")
    print(line("plain", series["plain"]))
    print(line("nms", series["nms"]))
    print(f"    graph nodes: {plain.n_nodes} without, {with_nms.n_nodes} with the stage "
          f"(+{(with_nms.n_nodes or 0) - (plain.n_nodes or 0)})")
