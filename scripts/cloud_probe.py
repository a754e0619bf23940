"""Time of the device mesh evaluation (cnrma_amd.cloud / csrc/cloud.hip) against the host path on the same clouds:
python scripts/cloud_probe.py [--out FILE.json] [--boxes N] [--reps R]

Clouds: the marching-cubes vertices of a synthetic room TSDF (synth.room_tsdf) at 192x192x80 and 192^3 as the prediction, and a
copy with a fifth of the points removed and the rest jittered by about 1 cm as the ground truth.  Per shape, in a child process of
its own under a time limit (the parent never opens the GPU):
  device  medians over repeated launches, by HIP events, of: down-sample (both clouds), grid build and query in each direction, the
          queries at each candidate search cell; the mean shells and candidates per query; modelled bytes per stage and their time
          at 8 TB/s
  host    the oracle's down-sample (tests/cloud_oracle.py) and scipy's cKDTree (build + query with 16 workers), wall clock
The gate: down-sample + build + query, both directions, takes less time on the device than on the host in the same run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((192, 192, 80), (192, 192, 192))
CELLS = (0.02, 0.04, 0.08)
VOXEL, THRESHOLD = 0.02, 0.05
HBM_BYTES_PER_S = 8e12
CASE_TIME_LIMIT_S = 240


def _median_us(fn, reps, warmup=3):
    import torch
    out = []
    for r in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def probe(dims, boxes, reps):
    import numpy as np
    import torch
    from scipy.spatial import cKDTree

    import cloud_oracle as CO
    from cnrma_amd import _lib, cloud, mesh, synth
    from cnrma_amd._lib import call, ptr, stream
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    vol = synth.room_tsdf(dims, boxes=boxes, seed=0)[0, 0].to(dev).contiguous()
    pred = mesh.marching_cubes(vol, 0.04).vertices.contiguous()
    g = torch.Generator(device="cpu").manual_seed(0)
    keep = torch.rand(len(pred), generator=g) >= 0.2
    gt = (pred.cpu()[keep] + torch.randn(int(keep.sum()), 3, generator=g) * 0.006).to(dev).contiguous()
    clouds = {"pred": pred, "gt": gt}
    lib = _lib.load()

    # ---- device: down-sample -----------------------------------------------------------------------------------
    ds, t_us, bytes_model = {}, {}, {}
    for name, p in clouds.items():
        n = len(p)
        nbytes = lib.cnrma_cloud_downsample_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)

        def run(p=p, n=n, ws=ws, nbytes=nbytes, out=out, info=info):
            call("cnrma_cloud_voxel_downsample_f32", ptr(p), n, None, VOXEL, ptr(ws), nbytes, ptr(out), None, n, ptr(info), stream())

        t_us[f"down_sample_{name}"] = _median_us(run, reps)
        v, flags = _lib.read_ints(info)[:2]
        assert flags == 0
        ds[name] = (out, info[:1], v)
        # points read three times (box, keys, means), (key, index) pairs written and read once each way by the sort at the least
        bytes_model[f"down_sample_{name}"] = 3 * 12 * n + 2 * 12 * n + 12 * v

    # ---- device: build + query per direction and candidate cell -------------------------------------------------
    per_cell = {}
    for cell in CELLS:
        row = {}
        for qn, tn in (("pred", "gt"), ("gt", "pred")):
            (q, nq_dev, nq), (t, nt_dev, nt) = ds[qn], ds[tn]
            nbytes = lib.cnrma_cloud_nn_workspace_bytes(len(t))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            dist = torch.empty(len(q), dtype=torch.float64, device=dev)
            idx = torch.empty(len(q), dtype=torch.int32, device=dev)
            stats = torch.zeros(2, dtype=torch.int64, device=dev)

            def build():
                call("cnrma_cloud_nn_build_f32", ptr(t), len(t), ptr(nt_dev), cell, ptr(ws), nbytes, stream())

            def query(s=None):
                call("cnrma_cloud_nn_query_f32", ptr(q), len(q), ptr(nq_dev), len(t), ptr(ws), ptr(dist), ptr(idx), ptr(s), stream())

            row[f"build_{tn}_us"] = _median_us(build, reps)
            row[f"query_{qn}_to_{tn}_us"] = _median_us(query, reps)
            query(stats)
            shells, cands = _lib.read_ints(stats)
            row[f"shells_per_query_{qn}_to_{tn}"] = shells / nq
            row[f"candidates_per_query_{qn}_to_{tn}"] = cands / nq
            # the build reads the live targets three times, writes and sorts (cell, index) pairs, writes 16-byte records and clears,
            # counts and scans the cell starts; a query reads its point, writes 12 bytes and reads 16 bytes per candidate
            row[f"build_{tn}_bytes"] = 3 * 12 * nt + 2 * 8 * nt + 16 * nt
            row[f"query_{qn}_to_{tn}_bytes"] = 24 * nq + 16 * cands
        row["queries_us"] = row["query_pred_to_gt_us"] + row["query_gt_to_pred_us"]
        row["builds_us"] = row["build_gt_us"] + row["build_pred_us"]
        per_cell[str(cell)] = row
    best_cell = min(CELLS, key=lambda c: per_cell[str(c)]["queries_us"])
    default = cloud.default_cell(THRESHOLD, VOXEL)
    d = per_cell[str(default)]
    device_us = t_us["down_sample_pred"] + t_us["down_sample_gt"] + d["builds_us"] + d["queries_us"]
    device_bytes = sum(bytes_model.values()) + sum(v for k, v in d.items() if k.endswith("_bytes"))

    # ---- host: the oracle's down-sample and cKDTree with 16 workers ------------------------------------------------
    hp, hg = pred.cpu().numpy(), gt.cpu().numpy()
    t0 = time.perf_counter()
    dp, dg = CO.down_sample(hp, VOXEL)[0], CO.down_sample(hg, VOXEL)[0]
    t1 = time.perf_counter()
    d_pg = cKDTree(dg.astype(np.float64)).query(dp.astype(np.float64), workers=16)[0]
    d_gp = cKDTree(dp.astype(np.float64)).query(dg.astype(np.float64), workers=16)[0]
    t2 = time.perf_counter()
    assert len(dp) == ds["pred"][2] and len(dg) == ds["gt"][2]
    m = cloud.eval_mesh(pred, gt, THRESHOLD, VOXEL)
    assert abs(m["dist1"] - d_pg.mean()) <= 1e-12 * d_pg.mean() and abs(m["dist2"] - d_gp.mean()) <= 1e-12 * d_gp.mean()
    host_us = (t2 - t0) * 1e6
    return dict(dims=list(dims), points_pred=len(pred), points_gt=len(gt), voxels_pred=ds["pred"][2], voxels_gt=ds["gt"][2], reps=reps,
                **{k + "_us": v for k, v in t_us.items()}, **{k + "_bytes": v for k, v in bytes_model.items()}, cells=per_cell,
                default_cell=default, fastest_cell=best_cell, device_total_us=device_us, device_bytes=device_bytes,
                device_us_at_8TBps=device_bytes / HBM_BYTES_PER_S * 1e6,
                memory_bound_fraction=device_bytes / HBM_BYTES_PER_S * 1e6 / device_us,
                host_down_sample_us=(t1 - t0) * 1e6, host_ckdtree_16_workers_us=(t2 - t1) * 1e6, host_total_us=host_us,
                device_faster_than_host=bool(device_us < host_us), metrics=m)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--boxes", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--case", type=int, default=None, help="(internal) probe SHAPES[case] in this process and print its JSON row")
    args = ap.parse_args()
    if args.case is not None:
        print("ROW " + json.dumps(probe(SHAPES[args.case], args.boxes, args.reps)))
        sys.exit(0)
    rows = []
    for case in range(len(SHAPES)):                               # a fresh child per shape, each under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(case), "--boxes", str(args.boxes), "--reps",
                            str(args.reps)], capture_output=True, text=True, timeout=CASE_TIME_LIMIT_S)
        if r.returncode != 0:
            sys.exit(f"case {case} failed with status {r.returncode}:\n{r.stdout}\n{r.stderr}")       # nothing more runs on the GPU
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")][-1][4:]))
        print(json.dumps(rows[-1]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r["device_faster_than_host"] for r in rows):
        sys.exit("the device path is not faster than the host path")
