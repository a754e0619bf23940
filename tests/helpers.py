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


# ---------------------------------------------------------------------------------------------------------------------
# depth-mode edge fixture (tests/golden/make_golden.py run_depth_edges; tests/test_rma_depth_edges_*.py)
# ---------------------------------------------------------------------------------------------------------------------
def look_at_projection(eye, target, f, cx, cy, up=(0.0, 0.0, 1.0)):
    """[3,4] fp32 projection K @ [R | -R eye] in full-resolution pixels of a pinhole camera at `eye` looking at `target`
    (camera rows right, down, forward; `up` must not be parallel to the viewing direction)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return torch.from_numpy((K @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)).astype(np.float32))


DEPTH_EDGES = "depth_edges"
DEPTH_EDGE_VIEWS = dict(inside=0, far15=1, miss=2, far25=3, axis=4)        # view order of the fixture
DEPTH_EDGE_KS = (0, 1, 2, 3, 4)


def depth_oracle_views(g, feats, tsdf, k, n_steps=None, projection=None, proj_inv=None):
    """the oracle's depth rows of every view of a depth_edges-like scene (ray parameters pinned through proj_inv; no one-row
    quirk: what rma_view_rows returns): (rows [M, 4+C] numpy, per-view counts, per-view debug dicts)"""
    from oracle import rma_oracle as O
    H, W = feats.shape[-2:]
    projection = t(g["projection"]) if projection is None else projection
    proj_inv = t(g["proj_inv"]) if proj_inv is None else proj_inv
    rows, counts, dbgs = [], [], []
    for v in range(feats.shape[0]):
        ps = O.scale_projection(projection[v], g["stride"])
        r, dbg = O.rma_depth_view(ps, feats[v], tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"] if n_steps is None else n_steps,
                                  k, o_d=O.ray_params(ps, H, W, proj_inv[v]), reference_quirks=False, return_debug=True)
        counts.append(0 if r is None else r.shape[0])
        dbgs.append(dbg)
        if r is not None:
            rows.append(r)
    return (torch.cat(rows) if rows else torch.zeros(0, 4 + feats.shape[1])).numpy(), counts, dbgs


def depth_last_step_variant(g):
    """the one geometry in which a ray's LAST sample is still inside the grid (t_max is the grid's diagonal): a camera just
    inside the outer corner of voxel (0,0,0) looking at the opposite corner, on a TSDF that is negative everywhere.  A ray that
    stays inside for all N steps has no sign change -- the product appended at N-1 is 1 (:876-878), not tsdf * "outside" --
    and gives no row; the rays beside it leave the grid early and hit there.  Returns (projection [1,3,4], tsdf [X,Y,Z])."""
    dims, vs, org, s = g["dims"], g["voxel_size"], np.array(g["origin"], np.float64), g["stride"]
    H, W = g["features"].shape[-2:]
    corner = org - 0.5 * vs
    proj = look_at_projection(corner + 0.05 * vs, corner + vs * np.array(dims, np.float64), s * 100.0, s * (W // 2), s * (H // 2))
    return proj.view(1, 3, 4), torch.full(dims, -0.5)


def depth_last_step_facts(g, k=4):
    """(rays whose N samples are all inside the grid and that have no hit, rays that hit) of depth_last_step_variant"""
    proj, tsdf = depth_last_step_variant(g)
    pinv = t(g["proj_inv_last_step"])
    _, _, dbg = depth_oracle_views(g, t(g["features"][:1]), tsdf, k, projection=proj, proj_inv=pinv)
    inside = dbg[0]["valid"].all(dim=1)
    return int((inside & ~dbg[0]["hit"]).sum()), int(dbg[0]["hit"].sum())


def depth_edge_facts(g):
    """what the depth_edges fixture is for, re-derived from its inputs with the oracle.  Every count but `miss_hits` must be
    non-zero: rays of the inside view whose first sign change is at step 0, and their slots with sel < 0 at k = 4; hits of the
    far views at N-2 and N-3, and their slots with sel >= N at k = 2; hit rays that enter the grid straight into a voxel with
    tsdf <= 0 (the change sits at the step before entry); rays of the axis view with an exactly-zero direction component, and
    its hits; rays that sample a NaN voxel, and hit rays with a NaN sample before their first change (a NaN product is no
    change); first changes whose product is zero through a +0.0 and through a -0.0 voxel; rays that sample a voxel of
    exactly 1.0 (the value that also stands for "outside")"""
    N = g["n_steps"]
    feats, tsdf = t(g["features"]), t(g["tsdf"])
    vw = DEPTH_EDGE_VIEWS
    _, _, d4 = depth_oracle_views(g, feats, tsdf, 4)
    _, _, d2 = depth_oracle_views(g, feats, tsdf, 2)
    f = dict(enter_nonpositive=0, nan_rays=0, nan_before_change=0, change_on_pos_zero=0, change_on_neg_zero=0, one_sampled=0)
    steps = torch.arange(N).view(1, -1)
    for dbg in d4:
        hit, best, sdf, valid = dbg["hit"], dbg["best"], dbg["sdf"], dbg["valid"]
        r = torch.nonzero(hit)[:, 0]
        b = best[r]
        f["enter_nonpositive"] += int((~valid[r, b] & valid[r, b + 1] & (sdf[r, b + 1] <= 0)).sum())
        nan = valid & torch.isnan(sdf)
        f["nan_rays"] += int(nan.any(dim=1).sum())
        f["nan_before_change"] += int((hit & (nan & (steps <= best.view(-1, 1))).any(dim=1)).sum())
        pair = torch.stack((sdf[r, b], sdf[r, b + 1]), dim=1)
        zero, neg = pair == 0, torch.signbit(pair)
        f["change_on_pos_zero"] += int((zero & ~neg).any(dim=1).sum())
        f["change_on_neg_zero"] += int((zero & neg).any(dim=1).sum())
        f["one_sampled"] += int((valid & (sdf == 1.0)).any(dim=1).sum())
    i, a = d4[vw["inside"]], d4[vw["axis"]]
    f["inside_best0"] = int((i["hit"] & (i["best"] == 0)).sum())
    f["inside_sel_below0"] = int((i["hit"].view(-1, 1) & (i["sel"] < 0)).sum())
    f["far15_at_Nm2"] = int((d4[vw["far15"]]["hit"] & (d4[vw["far15"]]["best"] == N - 2)).sum())
    f["far25_at_Nm3"] = int((d4[vw["far25"]]["hit"] & (d4[vw["far25"]]["best"] == N - 3)).sum())
    f["far25_at_Nm2"] = int((d4[vw["far25"]]["hit"] & (d4[vw["far25"]]["best"] == N - 2)).sum())
    f["far_sel_from_N"] = sum(int((d2[vw[n]]["hit"].view(-1, 1) & (d2[vw[n]]["sel"] >= N)).sum()) for n in ("far15", "far25"))
    f["axis_zero_dir"] = int((a["d"] == 0).any(dim=0).sum())
    f["axis_hits"] = int(a["hit"].sum())
    f["miss_hits"] = int(d4[vw["miss"]]["hit"].sum())
    return f
