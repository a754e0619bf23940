"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["tiny", "tiny_boxes_origin", "mini_p", "edge_empty_view", "edge_outside_axis", "edge_cropped_c12"]
# scenes whose grid border runs through free space, with cameras outside / on a lattice plane and axis-aligned rays
EDGE_SCENES = ["edge_outside_axis", "edge_cropped_c12"]
# scenes in which a view keeps exactly one sample and the reference drops it (ray_marching.py:781-782 / :930-931 inside the
# bare except of :277-287): their fixtures hold per-view rows only for the views the reference kept, so they are not in
# SCENES; dedicated tests use them (make_golden.py run_quirk_scene)
QUIRK_SCENES = ["edge_single_sample", "edge_single_sample_v1", "edge_single_sample_depth"]
QUIRK_SINGLE_VIEW = "edge_single_sample_only"      # its one view keeps one sample: the reference raises TypeError (:300)


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, f"rma_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["dims"] = tuple(int(x) for x in g["dims"])
    g["voxel_size"] = float(g["voxel_size"])
    g["stride"] = int(g["stride"])
    g["thr"] = float(g["thr"])
    g["n_steps"] = int(g["n_steps"])
    g["origin"] = tuple(float(x) for x in g["origin"])
    return g


def t(a, device=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(device) if device is not None else x


def bits_equal(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.dtype.kind == "f":
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))
    return a == b


def count_mismatch(a, b):
    return int(np.count_nonzero(~bits_equal(a, b)))


def fill_state_deterministic(module):
    """every floating tensor of the state dict <- a function of its KEY only (golden tests of networks too large to keep
    their weights as fixtures: the reference-side generator and the test fill both models identically)"""
    import zlib
    with torch.no_grad():
        for k, v in sorted(module.state_dict().items()):
            if not v.dtype.is_floating_point:
                continue
            g = torch.Generator().manual_seed(zlib.crc32(k.encode()))
            r = torch.randn(v.shape, generator=g)
            if k.endswith("running_var"):
                r = r.abs() * 0.5 + 0.5
            elif k.endswith("norm.weight"):
                r = 1.0 + 0.1 * r
            elif k.endswith(("norm.bias", "running_mean", ".bias")):
                r = 0.1 * r
            else:
                fan_in = max(1, v[0].numel()) if v.dim() > 1 else 1
                r = r * (2.0 / fan_in) ** 0.5
            v.copy_(r)
    return module


def elementwise_error(got, exp):
    """worst over the elements of min(|got - exp|, |got - exp| / |exp|): "within tol absolutely OR relatively", the north
    star's criterion for fp32 outputs (parity tolerances)"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    err = np.abs(got - exp)
    worst = np.minimum(err, err / np.maximum(np.abs(exp), 1e-300))
    return float(worst.max()) if worst.size else 0.0


def edge_facts(g):
    """what the edge fixtures (make_golden.py edge_outside_axis / edge_cropped_c12) are for, re-derived from their inputs with
    the oracle (ray parameters pinned through the fixture's proj_inv): counts of rays with an exactly-zero direction
    component, of rays that start outside the grid and enter it, of rays whose last kept NeuS sample is their last in-grid
    sample before they leave through free space, of view-0 depth hits at the step before entry, of voxels with camera
    depth <= 0 (== 0), of in-grid samples on the rounding tie x/vs = -0.5; the smallest distance of a NeuS weight of an
    in-grid sample to thr, and the number of views that keep exactly one sample"""
    from oracle import rma_oracle as O
    dims, vs, origin, N, thr, stride = g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"], g["stride"]
    feats, tsdf = g["features"], t(g["tsdf"])
    V, _, H, W = feats.shape
    org = torch.tensor(origin, dtype=torch.float32).view(3, 1, 1)
    f = dict(zero_dir=0, start_outside=0, exit_free=0, depth_before_entry=0, depth_le0=0, depth_eq0=0, tie=0,
             thr_margin=float("inf"), single_views=0)
    idx = O.voxel_coordinates(dims)
    world = torch.cat((idx.float() * vs + org.view(3, 1), torch.ones(1, idx.shape[1])), dim=0)
    for v in range(V):
        ps = O.scale_projection(t(g["projection"][v]), stride)
        cz = O.matmul_fma_chain(ps, world)[2]
        f["depth_le0"] += int((cz <= 0).sum())
        f["depth_eq0"] += int((cz == 0).sum())
        o, d = O.ray_params(ps, H, W, t(g["proj_inv"][v]))
        f["zero_dir"] += int((d == 0).any(dim=0).sum())
        place, _, valid, sdf = O.march_samples(o, d, tsdf, dims, vs, origin, N)
        f["start_outside"] += int((~valid[:, 0] & valid.any(dim=1)).sum())
        f["tie"] += int((((place - org) / vs == -0.5).any(dim=0) & valid).sum())
        # NeuS weights before the threshold (neus_weights, :757-763)
        s = torch.sigmoid(-sdf)
        alpha = torch.clamp((s - torch.cat((s[:, 1:], s[:, -1:]), dim=1)) / s, min=0)
        T_next = torch.cumprod(1 - alpha, dim=1)
        w = torch.cat((torch.ones_like(T_next[:, :1]), T_next[:, :-1]), dim=1) * alpha
        f["thr_margin"] = min(f["thr_margin"], float((w[valid].double() - thr).abs().min()))
        keep = valid & (w >= thr)
        f["single_views"] += int(keep.sum()) == 1
        steps = torch.arange(N).expand_as(keep)
        last = torch.where(keep, steps, -1).max(dim=1).values                      # last kept step per ray (-1: none)
        last_valid = torch.where(valid, steps, -1).max(dim=1).values               # last in-grid step per ray
        ray = torch.nonzero(last >= 0)[:, 0]
        n = last[ray]
        f["exit_free"] += int(((n == last_valid[ray]) & (n + 1 < N) & (sdf[ray, n] < 0)).sum())
        if v == 0:                                                                  # depth rows are stored for view 0
            prod = torch.cat((sdf[:, :-1] * sdf[:, 1:], torch.ones(sdf.shape[0], 1)), dim=1)
            change = prod <= 0
            best = torch.argmax(change.float(), dim=1)
            hit = change.any(dim=1) & (best + 1 < N)
            r = torch.nonzero(hit)[:, 0]
            f["depth_before_entry"] += int((~valid[r, best[r]] & valid[r, best[r] + 1]).sum())
    return f


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm + activation inputs whose pre-activation stays clear of the ReLU / ELU kink (tests/test_sparse_backward_edges_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
def clear_of_kink(x, w, b, eps, residual, act, margin=0.05):
    """fp32 (x, b, residual) whose fp64 pre-activation bn(x) * w + b [+ residual] has no element within `margin` of 0, so that an
    fp32 kernel and the fp64 reference take the same branch of the activation at EVERY element (nothing is masked out of a
    comparison).  With a residual the close elements of the residual move; without one a single bias per column cannot clear
    a thousand rows, so the close elements of x move (and the bias of a constant column, whose x cannot matter)."""
    from oracle import sparse_oracle as SO
    x, b = np.array(x), np.array(b, dtype=np.float32)          # x keeps its type where only the residual moves
    residual = None if residual is None else np.array(residual, dtype=np.float32)
    if act is None:
        return x, b, residual
    pre = SO.batch_norm_train(x, w, b, eps, residual, act)[1]["pre"]
    if residual is not None:
        near = np.abs(pre) < margin
        residual[near] += np.where(pre >= 0, 2 * margin, -2 * margin)[near].astype(np.float32)
    else:
        x = x.astype(np.float32)
        flat = x.astype(np.float64).var(0) == 0
        b[flat & (np.abs(b) < 2 * margin)] = 3 * margin
        if x.shape[0] <= 8:             # a few rows (two rows are always xhat = -1, +1): here a bias per column does clear them
            xw = SO.batch_norm_train(x, w, 0 * b, eps, None, act)[1]["pre"]
            cand = np.concatenate((b[None], np.repeat(np.linspace(-2, 2, 81, dtype=np.float32)[:, None], len(b), axis=1)))
            gap = np.abs(xw[None] + cand[:, None, :]).min(axis=1)                   # [candidate, column]
            gap[0] = np.where(gap[0] >= 2 * margin, np.inf, gap[0])                 # the bias given stays where it is clear already
            b = np.where(flat, b, cand[gap.argmax(axis=0), np.arange(len(b))]).astype(np.float32)
        for _ in range(100):
            st = SO.batch_norm_train(x, w, b, eps, None, act)[1]
            pre = st["pre"]
            near = (np.abs(pre) < margin) & ~flat
            if not near.any():
                break
            slope = np.asarray(w, dtype=np.float64) / np.sqrt(st["var"] + eps)
            step = (np.where(pre >= 0, 1.6 * margin, -1.6 * margin) - pre) / slope
            x[near] = (x.astype(np.float64) + step)[near].astype(np.float32)
    pre = SO.batch_norm_train(x, w, b, eps, residual, act)[1]["pre"]
    assert np.abs(pre).min() >= 0.8 * margin, np.abs(pre).min()
    return x, b, residual


# ---------------------------------------------------------------------------------------------------------------------
# sparse tensors whose capacity exceeds their live row count (tests/test_sparse_edges_gpu.py)
# ---------------------------------------------------------------------------------------------------------------------
POISON = 3e38           # a dead feature / residual value: finite, safe to read, and 3e38 * anything visible in any sum or maximum


def poison_coords(c, cap, step=1):
    """coordinates [cap, 4] whose rows >= len(c) are poison: copies of the live rows shifted by one voxel of the lattice
    (`step`) along x -- in range, duplicates of one another and neighbours of live rows, so a builder that reads one of them
    makes a duplicate or a false neighbour.  A shift that would leave +-32767 goes the other way."""
    c = np.asarray(c, dtype=np.int64)
    live = len(c)
    out = np.zeros((cap, 4), dtype=np.int64)
    out[:live] = c
    if live and cap > live:
        dead = c[np.arange(cap - live) % live].copy()
        dead[:, 1] += np.where(dead[:, 1] + step > 32766, -step, step)
        out[live:] = dead
    return out


def poison_rows(a, cap, device, value=POISON):
    """device tensor [cap, C]: the rows of `a` followed by rows of `value` (built on the device: capacities reach 250 000)"""
    a = torch.as_tensor(a, dtype=torch.float32)
    out = torch.full((cap, a.shape[1]), value, dtype=torch.float32, device=device)
    out[:a.shape[0]] = a.to(device)
    return out


def capacity_tensor(c, f, ts, device, cap=None, value=POISON, n_batch=None, compact=False):
    """SparseTensor of the rows (c, f) at tensor stride ts.  cap None / == len(c): an exact-size set (no live word, what the eager
    wrappers build); cap > len(c): CoordSet(n=cap, n_dev=live word) with poisoned coordinates and features behind the live
    rows -- what a static trace hands every kernel"""
    from cnrma_amd import sparse as S
    live = len(c)
    nb = int(n_batch if n_batch is not None else (np.asarray(c)[:, 0].max() + 1 if live else 1))
    if cap is None or cap == live:
        cs = S.CoordSet(torch.from_numpy(np.asarray(c).astype(np.int32)).to(device), ts, n_batch=nb)
        F = torch.as_tensor(f, dtype=torch.float32).to(device)
    else:
        assert cap > live
        n_dev = torch.tensor([live], dtype=torch.int32, device=device)
        cs = S.CoordSet(torch.from_numpy(poison_coords(c, cap, ts).astype(np.int32)).to(device), ts, n_batch=nb, n=cap, n_dev=n_dev)
        F = poison_rows(f, cap, device, value)
    cs.compact = compact
    return S.SparseTensor(F, cs)
