"""Indoor mAP: the host evaluator (postprocess.indoor_eval) against the device evaluator (postprocess.indoor_eval_device) on one
synthetic set of ScanNet-val size.

    python scripts/eval_probe.py --rounds=5 [--dets=1000] [--gts=30]

Set: 312 scenes, 18 classes, thresholds (0.25, 0.5), axis-aligned boxes.  Per scene `gts` ground-truth boxes (uniform classes,
centres in an 8 m x 8 m x 2 m room, sizes 0.4 .. 1.2 m) and `dets` detections: jittered copies of random ground-truth boxes, one
in ten with a random class, scores uniform in (0.01, 1) -- the load a score threshold of 0.01 leaves behind the NMS.
Timed with the host clock around a call that ends synchronised (both evaluators return host floats):

    host      indoor_eval: per threshold, class and scene two uploads, one IoU launch, one read-back, a Python loop per detection
    device    indoor_eval_device: one upload, two stable sorts, cnrma_eval_result_f32 (five launches), two reads
    result    DetectionEvaluator.result() alone on the already uploaded set (what a validation hook pays at the end of an epoch)

`same`: equal AP list lengths and every AP / recall within 1e-9.  Reads: calls of _lib.read_ints and Tensor.cpu inside one
indoor_eval_device call.  The host evaluator runs `--host-rounds` times (default 1: it takes seconds), the device forms `rounds`
times; medians, min .. max beside them."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cnrma_amd import _lib
from cnrma_amd import postprocess as PP
from cnrma_amd.evaluate import DetectionEvaluator


def option(name, default):
    for a in sys.argv[1:]:
        if a.startswith(f"--{name}="):
            return int(a.split("=")[1])
    return default


rounds, host_rounds = max(option("rounds", 5), 3), max(option("host-rounds", 1), 1)
n_scenes, n_classes, thrs = option("scenes", 312), 18, (0.25, 0.5)
dets, gts_per_scene = option("dets", 1000), option("gts", 30)
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)


def scene():
    gb = np.concatenate((rng.uniform(0, 8, (gts_per_scene, 2)), rng.uniform(0, 2, (gts_per_scene, 1)),
                         rng.uniform(0.4, 1.2, (gts_per_scene, 3))), axis=1).astype(np.float32)
    gl = rng.integers(0, n_classes, gts_per_scene)
    src = rng.integers(0, gts_per_scene, dets)
    db = gb[src].copy()
    db[:, :3] += rng.normal(0, 0.1, (dets, 3)).astype(np.float32)
    db[:, 3:] *= (1 + rng.normal(0, 0.12, (dets, 3)).clip(-0.5, 0.5)).astype(np.float32)
    dl = np.where(rng.random(dets) < 0.9, gl[src], rng.integers(0, n_classes, dets))
    return dict(boxes=gb, labels=gl), dict(boxes=db, scores=rng.uniform(0.01, 1, dets).astype(np.float32), labels=dl)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def line(name, xs):
    return f"{name:>8} {statistics.median(xs):11.3f} ms   ({min(xs):.3f} .. {max(xs):.3f}; {len(xs)} runs)"


pairs = [scene() for _ in range(n_scenes)]
gt_annos, dt_annos = [g for g, _ in pairs], [d for _, d in pairs]
print(f"eval_probe: {n_scenes} scenes x {dets} detections and {gts_per_scene} ground-truth boxes, {n_classes} classes, thresholds {thrs}; "
      f"{n_scenes * dets} detections, {n_scenes * gts_per_scene} boxes; device {torch.cuda.get_device_name(0)}")
host = lambda: PP.indoor_eval(gt_annos, dt_annos, thrs, n_classes=n_classes, device=dev)
device = lambda: PP.indoor_eval_device(gt_annos, dt_annos, thrs, n_classes=n_classes, device=dev)
got = device()                                              # warm-up (library load, allocator)
ev = DetectionEvaluator(n_classes, thrs, det_capacity=n_scenes * dets, gt_capacity=n_scenes * gts_per_scene,
                        scene_capacity=n_scenes, device=dev)
for g, d in pairs:
    ev.add(d["boxes"], d["scores"], d["labels"], g["boxes"], g["labels"])
added = ev.result()
reads = {"read_ints": 0, "Tensor.cpu": 0}
orig_read, orig_cpu = _lib.read_ints, torch.Tensor.cpu


def counting_read(t):
    reads["read_ints"] += 1
    return orig_read(t)


def counting_cpu(self, *a, **k):
    reads["Tensor.cpu"] += 1
    return orig_cpu(self, *a, **k)


_lib.read_ints, torch.Tensor.cpu = counting_read, counting_cpu
try:
    device()
finally:
    _lib.read_ints, torch.Tensor.cpu = orig_read, orig_cpu
series = dict(host=[], device=[], result=[])
for _ in range(host_rounds):
    ms, exp = wall(host)
    series["host"].append(ms)
for _ in range(rounds):
    series["device"].append(wall(device)[0])
    series["result"].append(wall(ev.result)[0])
same = all(len(got[k]) == len(exp[k]) if k.startswith("AP_") else True for k in exp) and all(
    np.allclose(np.asarray(got[k], np.float64), np.asarray(exp[k], np.float64), rtol=0, atol=1e-9) for k in exp)
for key in series:
    print(line(key, series[key]))
print(f"    same as the host: {same}; scene-by-scene add() gives the bulk upload's dict: {added == got}")
print(f"    device->host reads in indoor_eval_device: {reads}; library launches in result(): 5 (best, fill, claim, flag, ap)")
print("    " + ", ".join(f"{k} {v:.4f}" for k, v in exp.items() if not k.startswith("AP_")))
