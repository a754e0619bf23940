"""Time of the device mesh extraction (cnrma_amd.mesh / csrc/mesh.hip) on synthetic room TSDFs: python scripts/mesh_probe.py
[--out FILE.json] [--boxes N] [--reps R]

Times cnrma_mesh_count_f32 + cnrma_mesh_emit_f32 (the one device->host read of the counts between them is NOT in the window: the
counts are read once beforehand and the outputs sized from them), with HIP events around each repetition; reports the median and
the minimum.  Beside each time: the fraction of cells that are active, and the algorithmic bytes (the volume read once, vertices /
normals / faces written once) with the time they take at 8 TB/s."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import _lib, synth  # noqa: E402
from cnrma_amd._lib import call, ptr, stream  # noqa: E402

SHAPES = ((192, 192, 80), (192, 192, 192), (256, 256, 96))
HBM_BYTES_PER_S = 8e12


def probe(dims, boxes, reps, warmup=5):
    dev = torch.device("cuda:0")
    vol = synth.room_tsdf(dims, boxes=boxes, seed=0)[0, 0].to(dev).contiguous()
    X, Y, Z = dims
    nbytes = _lib.load().cnrma_mesh_workspace_bytes(X, Y, Z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    org = torch.zeros(3, dtype=torch.float32, device=dev)

    def count():
        call("cnrma_mesh_count_f32", ptr(vol), X, Y, Z, ptr(ws), nbytes, ptr(counts), stream())

    count()
    nv, nf, ncell, _ = _lib.read_ints(counts)
    vert = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    norm = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    face = torch.empty((nf, 3), dtype=torch.int32, device=dev)

    def emit():
        call("cnrma_mesh_emit_f32", ptr(vol), X, Y, Z, 0.04, ptr(org), ptr(ws), ptr(vert), ptr(norm), nv, ptr(face), nf, ptr(counts),
             stream())

    times = {"count": [], "emit": [], "both": []}
    for r in range(warmup + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        count()
        ev[1].record()
        emit()
        ev[2].record()
        ev[2].synchronize()
        if r >= warmup:
            times["count"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            times["emit"].append(ev[1].elapsed_time(ev[2]) * 1e3)
            times["both"].append(ev[0].elapsed_time(ev[2]) * 1e3)
    cells = (X - 1) * (Y - 1) * (Z - 1)
    algo = 4 * X * Y * Z + 24 * nv + 12 * nf
    return dict(dims=list(dims), vertices=nv, triangles=nf, active_cells=ncell, active_fraction=ncell / cells, workspace_bytes=nbytes,
                algorithmic_bytes=algo, us_at_8TBps=algo / HBM_BYTES_PER_S * 1e6, reps=reps,
                **{f"{k}_us_median": statistics.median(v) for k, v in times.items()},
                **{f"{k}_us_min": min(v) for k, v in times.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    _lib.require_gpu()
    rows = [probe(d, args.boxes, args.reps) for d in SHAPES]
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
