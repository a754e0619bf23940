"""Generate golden fixtures by running the REFERENCE's own Python (container only; needs /root/reference).

    python tests/golden/make_golden.py

Writes small .npz files next to this script. Each holds seeded inputs and the outputs of the reference
functions on the hot path. The script also asserts that oracle/rma_oracle.py reproduces every
output bit-for-bit -- that is what "the oracle is pinned" means for rows a1-a8 and a12.
Only data (inputs / expected outputs) is written; no reference source text goes into the repo.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import _ref_import as R  # noqa: E402
from cnrma_amd import synth  # noqa: E402
from oracle import rma_oracle as O  # noqa: E402


def eq(a, b, what):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a == b)
    assert same.all(), f"oracle != reference for {what}: {np.count_nonzero(~same)} of {a.size}"


def scene(shape, seed, boxes=0, origin=(0.0, 0.0, 0.0), V=None):
    sc = synth.make_scene(shape, seed=seed, boxes=boxes, V=V)
    if origin != (0.0, 0.0, 0.0):
        # shift the world frame: grid origin moves, cameras move with it
        sc["origin"] = origin
        t = torch.tensor(origin, dtype=torch.float32)
        P = sc["projection"].clone()
        P[..., 3] = P[..., 3] - (P[..., :3] @ t)
        sc["projection"] = P
    return sc


def ref_view_rows(fn, *args, **kw):
    """one view through the reference's ray_projection_neus / _depth the way aggregate_2d_features_ray_marching calls it
    (ray_marching.py:277-287): an exception skips the view.  A view that keeps exactly one sample raises TypeError
    (len() of the 0-dim index, :781-782 / :930-931).  Returns (rows or None, skipped)."""
    try:
        return fn(*args, **kw), False
    except TypeError:
        return None, True


def run_scene(rm, tr, name, sc, thr=0.05, n_steps=300, max_points=None, mask_seed=7):
    dims, vs, origin, stride = sc["dims"], sc["voxel_size"], sc["origin"], sc["stride"]
    feats, projs, tsdf = sc["features"], sc["projection"], sc["tsdf"]
    V = feats.shape[0]
    out = dict(features=feats[:, 0].numpy(), projection=projs[:, 0].numpy(), tsdf=tsdf[0, 0].numpy(),
               dims=np.array(dims), voxel_size=np.float64(vs), origin=np.array(origin, dtype=np.float32),
               stride=np.int64(stride), thr=np.float64(thr), n_steps=np.int64(n_steps))

    # ---- a2/a3 dense unprojection + accumulate + mean
    obj = R.make_raymarching(rm, dims, vs, origin, stride, thr=thr)
    for v in range(V):
        obj.aggregate_2d_features(projs[v], feats[v])
    vol0, valid0 = rm.backproject(dims, vs, obj.origin, O.scale_projection(projs[0], stride), feats[0])
    obj.clear_3d_features()
    o_vol, o_cnt = O.backproject_accum(dims, vs, origin, projs[:, 0], feats[:, 0], stride)
    eq(o_vol, obj.volume[0], "mean volume")
    eq(o_cnt > 0, obj.valid[0, 0], "valid")
    ov, ovalid, opx, opy = O.backproject_view(dims, vs, origin, O.scale_projection(projs[0, 0], stride), feats[0, 0])
    eq(ov.view(vol0.shape[1:]), vol0[0], "view-0 volume")
    eq(ovalid.view(valid0.shape[2:]), valid0[0, 0], "view-0 valid")
    out.update(dense_volume=obj.volume[0].numpy(), dense_count=o_cnt.numpy().astype(np.int32),
               view0_px=opx.numpy().astype(np.int64), view0_py=opy.numpy().astype(np.int64),
               view0_valid=ovalid.numpy())

    # ---- a4 ray parameters
    H, W = feats.shape[-2:]
    os_, ds_, pinvs = [], [], []
    for v in range(V):
        ps = O.scale_projection(projs[v], stride)
        o_ref, d_ref = rm.get_ray_parameter(ps, feats[v])
        o_or, d_or = O.ray_params(ps[0], H, W)
        eq(o_or, o_ref[0, :, 0], "o")
        eq(o_ref[0], o_or.view(3, 1).expand(3, H * W), "o constant over pixels")
        eq(d_or, d_ref[0], "d")
        os_.append(o_or.numpy()); ds_.append(d_or.numpy()); pinvs.append(O.projection_inverse(ps[0]).numpy())
    out.update(ray_o=np.stack(os_), ray_d=np.stack(ds_), proj_inv=np.stack(pinvs))

    # ---- a5 NeuS per view (+ debug intermediates of view 0)
    rows_all, counts = [], []
    for v in range(V):
        ps = O.scale_projection(projs[v], stride)
        ref, _ = ref_view_rows(obj.ray_projection_neus, ps, feats[v], tsdf, grids=n_steps, weight_threshold=thr)
        orc, dbg = O.rma_neus_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, n_steps, thr, return_debug=True)
        if ref is None:
            assert orc is None
            counts.append(0)
            continue
        eq(orc, ref[0], f"neus rows view {v}")
        rows_all.append(ref[0].numpy()); counts.append(ref[0].shape[0])
        if v == 0:
            out.update(v0_ray=dbg["ray"].numpy().astype(np.int32), v0_step=dbg["step"].numpy().astype(np.int16),
                       v0_w_full=dbg["w"].numpy(), v0_valid_full=np.packbits(dbg["valid"].numpy()),
                       v0_vid_kept=dbg["vid"][:, dbg["ray"], dbg["step"]].numpy().astype(np.int16))
    out.update(neus_rows=np.concatenate(rows_all) if rows_all else np.zeros((0, 4 + feats.shape[2]), np.float32),
               neus_counts=np.array(counts, dtype=np.int64))

    # ---- a7 aggregate (scene level)
    obj.points_detection = []
    obj.aggregate_2d_features_ray_marching(projs, feats, tsdf)
    pts_ref = obj.points_detection[0]
    pts_or = O.aggregate_rma(projs[:, 0], feats[:, 0], tsdf[0, 0], dims, vs, origin, stride, n_steps, thr)
    eq(pts_or, pts_ref, "aggregate points")
    out.update(points=pts_ref.numpy())

    # ---- a6 depth variant, k = 0, 1, 2 (view 0 and scene aggregate for k=1)
    for k in (0, 1, 2):
        ps = O.scale_projection(projs[0], stride)
        ref, _ = ref_view_rows(obj.ray_projection_depth, ps, feats[0], tsdf, grids=n_steps, select_grids=k)
        orc = O.rma_depth_view(ps[0], feats[0, 0], tsdf[0, 0], dims, vs, origin, n_steps, k)
        if ref is None:
            assert orc is None
            out[f"depth_rows_k{k}"] = np.zeros((0, 4 + feats.shape[2]), np.float32)
        else:
            eq(orc, ref[0], f"depth rows k={k}")
            out[f"depth_rows_k{k}"] = ref[0].numpy()

    # ---- a8 switch_pointcloud (test path) with the numpy-global-RNG mask
    mp = max_points or max(1, pts_ref.shape[0] // 3)
    obj.max_points = mp
    offset = torch.tensor([[0.37, -1.21, 0.05]])
    np.random.seed(mask_seed)
    c_ref, f_ref, _ = obj.switch_pointcloud([pts_ref], [None], offset, test=True)
    np.random.seed(mask_seed)
    mask = O.sample_mask_numpy(pts_ref.shape[0], mp)
    c_or, f_or = O.select_rows(pts_ref, offset[0], mask)
    eq(c_or, c_ref[0], "selected coords"); eq(f_or, f_ref[0], "selected feats")
    # a9 oracle voxelisation of that selection (ME semantics: parity unpinned; stored for regression only)
    Cq, Fq, src = O.voxelize(c_or, f_or, 0.01)
    out.update(sel_mask=np.packbits(mask), sel_max_points=np.int64(mp), sel_offset=offset[0].numpy(),
               sel_coords=c_ref[0].numpy(), sel_feats=f_ref[0].numpy(),
               vox_coords=Cq.numpy(), vox_src=src.numpy().astype(np.int32))
    np.savez_compressed(os.path.join(HERE, f"rma_{name}.npz"), **out)
    print(f"rma_{name}.npz: V={V} rows/view={counts} points={tuple(pts_ref.shape)} unique={Cq.shape[0]}")


# --------------------------------------------------------------------------------------------------------------------
# views that keep exactly ONE sample: the reference drops them (ray_marching.py:781-782 / :930-931 raise TypeError inside
# the bare except of :277-287); with no view left it raises TypeError itself (:300)
# --------------------------------------------------------------------------------------------------------------------
QUIRK_SHAPE = (3, 4, 30, 40, (48, 48, 20), 4)    # the "tiny" geometry with 4 channels: fixtures well under 100 KB


def rays_per_voxel(sc, v, n_steps=300):
    """int64 [X,Y,Z]: how many rays of view v take a valid sample in each voxel (O.march_samples)"""
    X, Y, Z = sc["dims"]
    H, W = sc["features"].shape[-2:]
    o, d = O.ray_params(O.scale_projection(sc["projection"][v, 0], sc["stride"]), H, W)
    _, vid, valid, _ = O.march_samples(o, d, sc["tsdf"][0, 0], sc["dims"], sc["voxel_size"], sc["origin"], n_steps)
    lin = (vid[0] * Y + vid[1]) * Z + vid[2]
    ray = torch.arange(lin.shape[0]).view(-1, 1).expand_as(lin)
    pairs = torch.unique(torch.stack((lin[valid], ray[valid])), dim=1)
    return torch.bincount(pairs[0], minlength=X * Y * Z).view(X, Y, Z)


def single_voxel(n_target, others=()):
    """linear id of a voxel sampled by exactly one ray of the target view (and by no ray of `others`): the middle one"""
    ok = n_target == 1
    for n in others:
        ok &= n == 0
    ids = torch.nonzero(ok.view(-1))[:, 0]
    return int(ids[ids.numel() // 2])


def quirk_neus_scene(target):
    """NeuS: the room of "tiny" (seed 4, 3 boxes) with every voxel that view `target` samples set to +1 except one voxel
    that exactly one of its rays samples, set to -1: that ray keeps one sample (alpha > 0 where it leaves the voxel), no
    other ray of the view keeps any -- the other views keep hundreds"""
    sc = synth.make_scene(QUIRK_SHAPE, seed=4, boxes=3, V=3)
    sc["features"] = torch.round(sc["features"] * 8) / 8          # values on a 1/8 grid: the fixture compresses well
    n = rays_per_voxel(sc, target)
    t = sc["tsdf"][0, 0]
    t.copy_(torch.round(t * 64) / 64)                              # and the TSDF on a 1/64 grid
    t[n > 0] = 1.0
    t.view(-1)[single_voxel(n)] = -1.0
    return sc


def quirk_depth_scene():
    """depth (select_grids = 0): TSDF +1 everywhere but a -1 block that only view 1 samples (its rays hit) and one -1 voxel
    that exactly one ray of view 0 and no ray of the others samples: view 0 keeps one row, views 1 and 2 keep hundreds"""
    sc = synth.make_scene(QUIRK_SHAPE, seed=6, V=3)
    sc["features"] = torch.round(sc["features"] * 8) / 8
    n0, n1, n2 = (rays_per_voxel(sc, v) for v in range(3))
    t = sc["tsdf"][0, 0]
    t.fill_(1.0)
    cand = (n1 > 0) & (n0 == 0)
    cx, cy, _ = torch.nonzero(cand).float().median(dim=0).values.long().tolist()
    box = torch.zeros_like(cand)
    box[max(0, cx - 3):cx + 3, max(0, cy - 3):cy + 3, :] = True
    t[cand & box] = -1.0
    t.view(-1)[single_voxel(n0, (n1, n2))] = -1.0
    return sc


def run_quirk_scene(rm, name, sc, thr=0.05, n_steps=300):
    """per view (NeuS, depth k = 0, 1, 2): the reference's rows, which views it skipped, and the one-row block of each
    skipped view from the oracle's pre-skip path (the product's rma_view_rows has no quirk and returns it); the scene
    aggregate of the reference's own aggregate_2d_features_ray_marching per mode, or a flag when it raises TypeError"""
    dims, vs, origin, stride = sc["dims"], sc["voxel_size"], sc["origin"], sc["stride"]
    feats, projs, tsdf = sc["features"], sc["projection"], sc["tsdf"]
    V, C = feats.shape[0], feats.shape[2]
    out = dict(features=feats[:, 0].numpy(), projection=projs[:, 0].numpy(), tsdf=tsdf[0, 0].numpy(),
               dims=np.array(dims), voxel_size=np.float64(vs), origin=np.array(origin, dtype=np.float32),
               stride=np.int64(stride), thr=np.float64(thr), n_steps=np.int64(n_steps),
               proj_inv=np.stack([O.projection_inverse(O.scale_projection(projs[v, 0], stride)).numpy() for v in range(V)]))
    summary = {}
    for mode, k in (("neus", None), ("depth", 0), ("depth", 1), ("depth", 2)):
        tag = "neus" if mode == "neus" else f"depth_k{k}"
        obj = R.make_raymarching(rm, dims, vs, origin, stride, rtype=mode, thr=thr, depth_points=k)
        rows, counts, skipped, single = [], [], [], []
        for v in range(V):
            ps = O.scale_projection(projs[v], stride)
            if mode == "neus":
                ref, skip = ref_view_rows(obj.ray_projection_neus, ps, feats[v], tsdf, grids=n_steps, weight_threshold=thr)
                orc = O.rma_neus_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, n_steps, thr)
                raw = O.rma_neus_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, n_steps, thr, reference_quirks=False)
            else:
                ref, skip = ref_view_rows(obj.ray_projection_depth, ps, feats[v], tsdf, grids=n_steps, select_grids=k)
                orc = O.rma_depth_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, n_steps, k)
                raw = O.rma_depth_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, n_steps, k, reference_quirks=False)
            if skip:                                   # the reference raised: the oracle drops the view, one raw row
                assert orc is None and raw is not None and raw.shape[0] == 1, (tag, v)
                single.append(raw.numpy())
            elif ref is None:
                assert orc is None and raw is None
            else:
                eq(orc, ref[0], f"{tag} rows view {v}")
                rows.append(ref[0].numpy())
            counts.append(0 if ref is None else ref[0].shape[0])
            skipped.append(skip)
        out[f"{tag}_counts"] = np.array(counts, dtype=np.int64)
        out[f"{tag}_skipped"] = np.array(skipped)
        out[f"{tag}_rows"] = np.concatenate(rows) if rows else np.zeros((0, 4 + C), np.float32)
        out[f"{tag}_single_rows"] = np.concatenate(single) if single else np.zeros((0, 4 + C), np.float32)
        # the scene aggregate, from the reference's own loop
        obj.points_detection = []
        try:
            obj.aggregate_2d_features_ray_marching(projs, feats, tsdf)
            pts_ref = obj.points_detection[0]
        except TypeError:
            pts_ref = None
        if pts_ref is None:
            try:
                O.aggregate_rma(projs[:, 0], feats[:, 0], tsdf[0, 0], dims, vs, origin, stride, n_steps, thr, mode, k or 0)
                raise AssertionError(f"{tag}: the oracle aggregates a scene the reference rejects")
            except TypeError:
                pass
            out[f"{tag}_raises"] = np.bool_(True)
            out[f"{tag}_points"] = np.zeros((0, 3 + C), np.float32)
        else:
            pts_or = O.aggregate_rma(projs[:, 0], feats[:, 0], tsdf[0, 0], dims, vs, origin, stride, n_steps, thr, mode, k or 0)
            eq(pts_or, pts_ref, f"{tag} aggregate points")
            out[f"{tag}_raises"] = np.bool_(False)
            out[f"{tag}_points"] = pts_ref.numpy()
        summary[tag] = [("skip" if s_ else c) for c, s_ in zip(counts, skipped)] + (["raises"] if pts_ref is None else [])
    path = os.path.join(HERE, f"rma_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"rma_{name}.npz: V={V} {summary} ({os.path.getsize(path)} bytes)")


def run_quirk_single_view(rm, name, sc, thr=0.05, n_steps=300):
    """one view that keeps exactly one sample: the reference's aggregate_2d_features_ray_marching raises TypeError (:300,
    no view left).  Only the inputs and that flag are saved."""
    dims, vs, origin, stride = sc["dims"], sc["voxel_size"], sc["origin"], sc["stride"]
    feats, projs, tsdf = sc["features"][:1], sc["projection"][:1], sc["tsdf"]
    obj = R.make_raymarching(rm, dims, vs, origin, stride, thr=thr)
    obj.points_detection = []
    try:
        obj.aggregate_2d_features_ray_marching(projs, feats, tsdf)
        raises = False
    except TypeError:
        raises = True
    assert raises, "the reference aggregated a scene whose only view keeps one sample"
    raw = O.rma_neus_view(O.scale_projection(projs[0, 0], stride), feats[0, 0], tsdf[0, 0], dims, vs, origin, n_steps, thr,
                          reference_quirks=False)
    assert raw is not None and raw.shape[0] == 1
    out = dict(features=feats[:, 0].numpy(), projection=projs[:, 0].numpy(), tsdf=tsdf[0, 0].numpy(),
               dims=np.array(dims), voxel_size=np.float64(vs), origin=np.array(origin, dtype=np.float32),
               stride=np.int64(stride), thr=np.float64(thr), n_steps=np.int64(n_steps),
               proj_inv=O.projection_inverse(O.scale_projection(projs[0, 0], stride)).numpy()[None],
               neus_raises=np.bool_(raises))
    path = os.path.join(HERE, f"rma_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"rma_{name}.npz: V=1 raises TypeError ({os.path.getsize(path)} bytes)")


# --------------------------------------------------------------------------------------------------------------------
# edge geometry: the border of the grid runs through free space (a scene larger than the grid, cut by it), cameras stand
# outside the grid, on a lattice plane and above a corner; axis-aligned rays with exactly-zero direction components; grazing
# rays on the rounding tie x/vs = -0.5; odd channel counts and odd map sizes
# --------------------------------------------------------------------------------------------------------------------
def projection_of(R, eye, f, cx, cy):
    """[3,4] fp32 K @ [R | -R eye] in full-resolution pixels (R: world -> camera rows right, down, forward)"""
    R, eye = np.asarray(R, np.float64), np.asarray(eye, np.float64)
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return torch.from_numpy((K @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)).astype(np.float32))


def look_at(eye, target):
    fwd = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(fwd, right), fwd])


def box_tsdf(dims, boxes, specks=(), speck_value=1.0):
    """free space (-1) everywhere but axis-aligned boxes (centre, half extents in voxels; TSDF = -signed distance / 3 voxels,
    clamped, on a 1/64 grid) and single-voxel specks of positive TSDF"""
    X, Y, Z = dims
    px, py, pz = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    d = np.full(dims, np.inf)
    for c, h in boxes:
        q = np.stack([np.abs(px - c[0]) - h[0], np.abs(py - c[1]) - h[1], np.abs(pz - c[2]) - h[2]])
        d = np.minimum(d, np.sqrt((np.maximum(q, 0) ** 2).sum(0)) + np.minimum(q.max(0), 0))
    tsdf = np.round(np.clip(-d / 3.0, -1.0, 1.0) * 64) / 64
    for s in specks:
        tsdf[s] = speck_value
    return torch.from_numpy(tsdf.astype(np.float32)).view(1, 1, X, Y, Z)


def edge_scene(dims, origin, stride, C, hw, projections, tsdf, seed):
    V = len(projections)
    g = torch.Generator().manual_seed(seed)
    feats = torch.round(torch.randn(V, 1, C, hw[0], hw[1], generator=g) * 8) / 8          # compresses well
    return dict(features=feats, projection=torch.stack(projections).view(V, 1, 3, 4), tsdf=tsdf, dims=tuple(dims),
                voxel_size=0.04, origin=tuple(origin), stride=stride)


EDGE_AXIS_DIMS, EDGE_AXIS_ORIGIN = (50, 45, 27), (-0.31, 0.173, -0.05)
EDGE_AXIS_SPECKS = ((9, 21, 14), (30, 21, 14), (41, 21, 14), (20, 8, 20), (44, 38, 4), (5, 40, 22))


def edge_axis_projections():
    """view 0: outside, 0.19 m beyond the low-x face, looking along +x (exact permutation, f = 64, principal point on the
    feature-map pixel (20, 15) at stride 4: the ray of that pixel runs along the axis, its row and column have exactly-zero
    direction components); view 1: inside, the eye on the lattice plane of column 23 (camera depth exactly 0 there, the
    columns below it behind the camera); view 2: above the high corner, oblique -- some rays miss the grid"""
    ox, oy, oz = EDGE_AXIS_ORIGIN
    R = [[0, -1, 0], [0, 0, -1], [1, 0, 0]]
    x23 = float((torch.tensor(23.0) * 0.04 + torch.tensor(ox, dtype=torch.float32)).item())      # fl(fl(23 vs) + ox)
    eye2 = np.array([ox + 50 * 0.04 + 0.15, oy + 45 * 0.04 + 0.2, oz + 27 * 0.04 + 0.35])
    return [projection_of(R, (-0.5, 1.0, 0.5), 64.0, 80.0, 60.0),
            projection_of(R, (x23, 1.0, 0.5), 64.0, 80.0, 60.0),
            projection_of(look_at(eye2, (ox + 0.9, oy + 0.8, oz + 0.3)), eye2, 64.0, 80.0, 60.0)]


def edge_outside_axis_scene():
    tsdf = box_tsdf(EDGE_AXIS_DIMS, [((38, 10, 8), (5, 4, 4)), ((12, 34, 18), (4, 5, 5)), ((33, 33, 6), (3, 2, 3))],
                    EDGE_AXIS_SPECKS)
    return edge_scene(EDGE_AXIS_DIMS, EDGE_AXIS_ORIGIN, 4, 8, (30, 40), edge_axis_projections(), tsdf, seed=21)


def edge_cropped_c12_scene():
    """stride 1, C = 12, 29 x 37 maps (H*W odd); view 0 stands half a voxel below the low-x face (fl(eye_x - ox) =
    -0.5 vs exactly) and looks along +y: the rays of pixel column 18 have dx = 0 and run in the plane x = ox - 0.5 vs, on
    the rounding tie of voxel column 0"""
    vs32 = np.float32(0.04)
    eye_x = np.float32(0.0)
    ox = np.float32(eye_x + np.float32(0.5) * vs32)
    assert np.float32(eye_x - ox) == -np.float32(0.5) * vs32
    origin = (float(ox), -0.1, 0.0)
    dims = (33, 20, 41)
    R = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    projs = [projection_of(R, (float(eye_x), -0.25, 0.75), 16.0, 18.0, 14.0),
             projection_of(look_at((0.75, 0.3125, 1.0), (0.2, 0.55, 0.3)), (0.75, 0.3125, 1.0), 16.0, 18.0, 14.0)]
    tsdf = box_tsdf(dims, [((8, 12, 10), (4, 3, 6)), ((24, 9, 30), (5, 4, 4)), ((16, 17, 2), (3, 5, 3))],
                    ((0, 10, 20), (0, 15, 26), (20, 5, 22), (28, 14, 12)))
    return edge_scene(dims, origin, 1, 12, (29, 37), projs, tsdf, seed=22)


def run_edge_scenes(rm, tr):
    run_scene(rm, tr, "edge_outside_axis", edge_outside_axis_scene())
    check_edge_fixture("edge_outside_axis")
    run_scene(rm, tr, "edge_cropped_c12", edge_cropped_c12_scene(), thr=0.03)
    check_edge_fixture("edge_cropped_c12", need_depth0=False, need_tie=True)


def check_edge_fixture(name, need_exit=True, need_entry=True, need_depth0=True, need_tie=False):
    """the fixture holds the edges it is for (tests/test_oracle_cpu.py re-derives the same facts)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from helpers import edge_facts, load_golden
    f = edge_facts(load_golden(name))
    print(f"rma_{name}.npz edges: {f}")
    assert f["zero_dir"] > 0 and f["start_outside"] > 0, (name, f)
    assert not need_exit or f["exit_free"] > 0, (name, f)
    assert not need_entry or f["depth_before_entry"] > 0, (name, f)
    assert f["depth_le0"] > 0 and (not need_depth0 or f["depth_eq0"] > 0), (name, f)
    assert not need_tie or f["tie"] > 0, (name, f)
    assert f["thr_margin"] > 1e-6, (name, f)              # no weight flips with the 1-ulp tail of the CPU sigmoid
    assert f["single_views"] == 0, (name, f)              # a one-sample view is the quirk case (QUIRK_SCENES)
    return f


# --------------------------------------------------------------------------------------------------------------------
# depth mode (ray_projection_depth, :809-956) at its edges, select_grids = 0..4: first sign changes at step 0 and at
# N-2 / N-3 (slots sel < 0 and sel >= N are masked, :899-900), rays that enter the grid straight into tsdf <= 0, rays with
# exactly-zero direction components, a view that misses the grid between views that hit, and voxels of exactly 0.0, -0.0,
# 1.0 and NaN under the `product <= 0` rule (:876-879)
# --------------------------------------------------------------------------------------------------------------------
DEPTH_EDGE_DIMS, DEPTH_EDGE_ORIGIN, DEPTH_EDGE_STEPS, DEPTH_EDGE_STRIDE = (12, 10, 7), (0.1, -0.2, 0.05), 40, 2
DEPTH_EDGE_HW, DEPTH_EDGE_C = (9, 13), 4
DEPTH_EDGE_PLANTED = (((4, 4, 3), 0.0), ((5, 5, 3), -0.0), ((5, 4, 4), float("nan")), ((4, 5, 3), 1.0), ((3, 4, 3), -0.0),
                      ((4, 3, 2), float("nan")), ((6, 4, 2), 0.0), ((3, 5, 4), 1.0), ((5, 4, 2), -0.0), ((4, 3, 4), 0.0))


def depth_edges_scene():
    """views: 0 inside the grid, next to a voxel border; 1 and 3 outside on the diagonal through the outer corner of voxel
    (0,0,0), 1.5 and 2.5 steps short of t_max = N t_one from it, long focal length; 2 looks away from the grid (no row: an
    empty view between views that hit); 4 below the grid looking exactly along +z, principal point on a pixel centre"""
    sys.path.insert(0, os.path.dirname(HERE))
    from helpers import look_at_projection
    X, Y, Z = DEPTH_EDGE_DIMS
    vs, s = 0.04, DEPTH_EDGE_STRIDE
    org = np.array(DEPTH_EDGE_ORIGIN)
    t_one = O.step_length(DEPTH_EDGE_DIMS, vs, DEPTH_EDGE_STEPS)
    g = torch.Generator().manual_seed(31)
    tsdf = torch.round((torch.rand(X, Y, Z, generator=g) * 2 - 1) * 64) / 64
    tsdf[tsdf == 0] = 1.0 / 64                                   # the only zeros are the planted ones
    tsdf = tsdf.clamp(-63.0 / 64, 63.0 / 64)
    tsdf[:3, :3, :3] = -0.5                                      # what the far cameras' rays enter the grid into
    for ijk, val in DEPTH_EDGE_PLANTED:
        tsdf[ijk] = val
    corner = org - 0.5 * vs
    diag = np.ones(3) / np.sqrt(3.0)
    H, W = DEPTH_EDGE_HW
    cx, cy = s * (W // 2), s * (H // 2)                           # principal point on the centre pixel of the feature map
    eye_in = org + vs * np.array([5.3, 4.45, 3.4])
    far = [corner - diag * (DEPTH_EDGE_STEPS - short) * t_one for short in (1.5, 2.5)]
    eye_axis = org + np.array([5 * vs, 4 * vs, -0.06])
    projs = [look_at_projection(eye_in, org + vs * np.array([1.0, 2.0, 1.5]), s * 7.0, cx, cy),
             look_at_projection(far[0], corner, s * 600.0, cx, cy),
             look_at_projection(org + np.array([-0.3, 0.1, 0.1]), org + np.array([-1.3, 0.0, 0.3]), s * 7.0, cx, cy),
             look_at_projection(far[1], corner, s * 600.0, cx, cy),
             look_at_projection(eye_axis, eye_axis + np.array([0.0, 0.0, 1.0]), s * 10.0, cx, cy, up=(0.0, -1.0, 0.0))]
    sc = edge_scene(DEPTH_EDGE_DIMS, DEPTH_EDGE_ORIGIN, s, DEPTH_EDGE_C, DEPTH_EDGE_HW, projs, tsdf.view(1, 1, X, Y, Z), seed=32)
    sc["n_steps"] = DEPTH_EDGE_STEPS
    return sc


def run_depth_edges(rm, name="depth_edges"):
    """per view and select_grids = 0..4: the reference's ray_projection_depth rows (oracle == reference asserted before
    anything is saved), the per-view row counts, and the scene aggregate of the reference's own
    aggregate_2d_features_ray_marching (its call of ray_projection_depth given the fixture's step count: the loop itself
    marches the default 300 steps)"""
    sc = depth_edges_scene()
    dims, vs, origin, stride, N = sc["dims"], sc["voxel_size"], sc["origin"], sc["stride"], sc["n_steps"]
    feats, projs, tsdf = sc["features"], sc["projection"], sc["tsdf"]
    V, C = feats.shape[0], feats.shape[2]
    H, W = feats.shape[-2:]
    pinv = [O.projection_inverse(O.scale_projection(projs[v, 0], stride)) for v in range(V)]
    out = dict(features=feats[:, 0].numpy(), projection=projs[:, 0].numpy(), tsdf=tsdf[0, 0].numpy(),
               dims=np.array(dims), voxel_size=np.float64(vs), origin=np.array(origin, dtype=np.float32),
               stride=np.int64(stride), thr=np.float64(0.05), n_steps=np.int64(N), proj_inv=np.stack([p.numpy() for p in pinv]))
    summary = {}
    for k in range(5):
        obj = R.make_raymarching(rm, dims, vs, origin, stride, rtype="depth", depth_points=k)
        rows, counts = [], []
        for v in range(V):
            ps = O.scale_projection(projs[v], stride)
            o_ref, d_ref = rm.get_ray_parameter(ps, feats[v])
            o_or, d_or = O.ray_params(ps[0], H, W, pinv[v])
            eq(o_or, o_ref[0, :, 0], f"o view {v}"); eq(d_or, d_ref[0], f"d view {v}")
            ref, skip = ref_view_rows(obj.ray_projection_depth, ps, feats[v], tsdf, grids=N, select_grids=k)
            orc = O.rma_depth_view(ps[0], feats[v, 0], tsdf[0, 0], dims, vs, origin, N, k, o_d=(o_or, d_or))
            assert not skip, (k, v)                            # a one-row view is the quirk fixtures' case
            if ref is None:
                assert orc is None, (k, v)
            else:
                eq(orc, ref[0], f"depth rows k={k} view {v}")
                rows.append(ref[0].numpy())
            counts.append(0 if ref is None else ref[0].shape[0])
        out[f"depth_k{k}_counts"] = np.array(counts, dtype=np.int64)
        out[f"depth_k{k}_rows"] = np.concatenate(rows)
        depth = obj.ray_projection_depth
        obj.ray_projection_depth = lambda *a, _depth=depth, **kw: _depth(*a, grids=N, **kw)
        obj.points_detection = []
        obj.aggregate_2d_features_ray_marching(projs, feats, tsdf)
        pts_ref = obj.points_detection[0]
        pts_or = O.aggregate_rma(projs[:, 0], feats[:, 0], tsdf[0, 0], dims, vs, origin, stride, N, mode="depth", select_grids=k,
                                 proj_inv=torch.stack(pinv))
        eq(pts_or, pts_ref, f"depth aggregate k={k}")
        out[f"depth_k{k}_points"] = pts_ref.numpy()
        summary[k] = counts
    # the last step inside the grid (helpers.depth_last_step_variant: its camera and TSDF are functions of the inputs above;
    # the maps are those of view 0): the inverse and the reference's rows
    from helpers import depth_edge_facts, depth_last_step_facts, depth_last_step_variant, load_golden
    proj_l, tsdf_l = depth_last_step_variant(dict(dims=dims, voxel_size=vs, origin=origin, stride=stride, features=out["features"]))
    ps = O.scale_projection(proj_l, stride)
    pinv_l = O.projection_inverse(ps[0])
    out["proj_inv_last_step"] = pinv_l.numpy()[None]
    obj = R.make_raymarching(rm, dims, vs, origin, stride, rtype="depth")
    for k in range(5):
        ref, skip = ref_view_rows(obj.ray_projection_depth, ps, feats[0], tsdf_l.view(1, 1, *dims), grids=N, select_grids=k)
        orc = O.rma_depth_view(ps[0], feats[0, 0], tsdf_l, dims, vs, origin, N, k, o_d=O.ray_params(ps[0], H, W, pinv_l))
        assert not skip and ref is not None
        eq(orc, ref[0], f"last-step rows k={k}")
        out[f"last_step_k{k}_rows"] = ref[0].numpy()
    path = os.path.join(HERE, f"rma_{name}.npz")
    np.savez_compressed(path, **out)
    g = load_golden(name)
    facts, last = depth_edge_facts(g), depth_last_step_facts(g)
    print(f"rma_{name}.npz: V={V} rows/view per k={summary} ({os.path.getsize(path)} bytes)\n  edges: {facts}\n"
          f"  last step: {last[0]} rays inside for all {N} steps without a hit, {last[1]} rays hit")
    assert facts["miss_hits"] == 0 and all(n > 0 for key, n in facts.items() if key != "miss_hits"), facts
    assert min(last) > 0, last


def run_decode(head_mod):
    """a12: _bbox_pred_to_bbox for the 6-DoF and the 8->7 'fcaf3d' yaw parametrisation + compute_centerness."""
    g = torch.Generator().manual_seed(3)
    h = head_mod.FCAF3DHead.__new__(head_mod.FCAF3DHead)
    n = 257
    pts = torch.rand(n, 3, generator=g) * 6
    out = dict(points=pts.numpy())
    for nreg, yaw in ((6, "fcaf3d"), (8, "fcaf3d"), (8, "sin-cos"), (7, "naive")):
        h.yaw_parametrization = yaw
        reg = torch.randn(n, nreg, generator=g)
        pred = torch.cat((torch.exp(reg[:, :6]), reg[:, 6:]), dim=1)
        box = h._bbox_pred_to_bbox(pts, pred)
        out[f"pred_{nreg}_{yaw}"] = pred.numpy()
        out[f"box_{nreg}_{yaw}"] = box.numpy()
    t = torch.rand(64, 7, generator=g) + 0.01
    out["centerness_in"] = t.numpy()
    out["centerness_out"] = head_mod.compute_centerness(t).numpy()
    np.savez_compressed(os.path.join(HERE, "decode.npz"), **out)
    print("decode.npz written")


# --------------------------------------------------------------------------------------------------------------------
# FCAF3D training targets and the composition of the three losses (fcaf3d_head.py:405-484, :142-214), boxes with yaw 0
# --------------------------------------------------------------------------------------------------------------------
ASSIGN_LIMIT, ASSIGN_TOPK = 27, 18


def save_stable(path, arrays):
    """np.savez_compressed with fixed member dates: numpy stamps every member with the wall clock, so its files differ from
    run to run; this one is the same bytes for the same arrays"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asarray(value), allow_pickle=False)


def cells(n, step):
    g = (torch.arange(n, dtype=torch.float32) + 0.5) * step
    return torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()


def gt_row(cx, cy, cz, dx, dy, dz):
    """(x, y, z_bottom, dx, dy, dz, yaw = 0) of the box with gravity centre (cx, cy, cz)"""
    return [cx, cy, cz - dz / 2, dx, dy, dz, 0.0]


class GTStandIn:
    """the three attributes of DepthInstance3DBoxes the reference's assigner reads (mmdet3d is absent): tensor [m, 7] =
    (x, y, z_bottom, dx, dy, dz, yaw), volume = dx dy dz, gravity_center = the bottom centre lifted by dz / 2"""

    def __init__(self, rows):
        self.tensor = torch.tensor(rows, dtype=torch.float32).view(-1, 7)
        self.volume = self.tensor[:, 3] * self.tensor[:, 4] * self.tensor[:, 5]
        self.gravity_center = self.tensor[:, :3].clone()
        self.gravity_center[:, 2] += self.tensor[:, 5] / 2

    def __len__(self):
        return len(self.tensor)


def rotation_stand_in(points, angles, axis=0):
    """rotation_3d_in_axis for boxes without yaw: the identity, whatever convention the third-party function follows"""
    assert (angles == 0).all(), "the assignment fixture holds boxes with yaw 0 only"
    return points


def ieee_sqrt(x):
    return torch.from_numpy(np.sqrt(x.detach().numpy()))


def assign_scenes():
    """name -> (levels, box rows, labels, limit, topk); every box has yaw 0 and a label of its own"""
    lattice = [cells(n, s) for n, s in ((12, .08), (6, .16), (3, .32), (2, .64))]
    rng = np.random.RandomState(11)
    random_levels = [torch.from_numpy(rng.uniform(0, 2, (n, 3)).astype(np.float32)) for n in (3001, 777, 130, 65)]
    random_rows = [gt_row(*rng.uniform(.3, 1.7, 3), *rng.uniform(.25, 1.4, 3)) for _ in range(5)]
    rng = np.random.RandomState(12)
    gap_levels = [torch.from_numpy(rng.uniform(0, 2, (n, 3)).astype(np.float32)) for n in (900, 0, 70, 9)]
    gap_rows = [gt_row(*rng.uniform(.5, 1.5, 3), *rng.uniform(.3, 1.6, 3)) for _ in range(4)]
    # the unit box around (1, 1, 1): three points on a face, one on a corner (a face distance of exactly 0: not inside), one
    # a single ulp inside.  Fewer than topk + 1 candidates, so every inside point of level 0 passes the k-th value of -1 -- a
    # face point taken for an inside point would become a positive row
    on_face = torch.tensor([[1.5, 1.0, 1.0], [0.5, 1.0, 1.25], [1.0, 1.0, 1.5], [1.5, 1.5, 1.5],
                            [float(np.nextafter(np.float32(1.5), np.float32(0))), 1.0, 1.0]])
    pts7 = cells(2, .3)[:7]
    return {
        # k-th-value ties (a box centred on a lattice plane), a box nested in it, a far box, the equal-volume duplicate
        "lattice": (lattice, [gt_row(.48, .48, .48, .64, .64, .64), gt_row(.40, .44, .45, .30, .30, .30),
                              gt_row(5.0, 5.0, 5.0, .50, .50, .50), gt_row(.48, .48, .48, .64, .64, .64)], [3, 7, 2, 5],
                    ASSIGN_LIMIT, ASSIGN_TOPK),
        # >= limit on every level (-> the last), < limit on level 0 (-> -1, clamped to 0), >= limit on levels 0 and 1 only (-> 1)
        "best_level": (lattice[:3], [gt_row(.48, .48, .48, 2.0, 2.0, 2.0), gt_row(.30, .30, .30, .17, .17, .17),
                                     gt_row(.60, .60, .60, .60, .60, .60)], [1, 2, 3], ASSIGN_LIMIT, ASSIGN_TOPK),
        # n = 7 < topk + 1, on three levels and on one
        "few_points": ([pts7[:4].clone(), pts7[4:6].clone(), pts7[6:].clone()], [gt_row(.3, .3, .3, 1.0, 1.0, 1.0)], [4],
                       ASSIGN_LIMIT, ASSIGN_TOPK),
        "few_points_one_level": ([pts7.clone()], [gt_row(.31, .27, .34, 1.0, 1.0, 1.0)], [4], ASSIGN_LIMIT, ASSIGN_TOPK),
        "random": (random_levels, random_rows, [6, 0, 17, 9, 12], ASSIGN_LIMIT, ASSIGN_TOPK),
        "random_top1_limit1": (random_levels, random_rows, [6, 0, 17, 9, 12], 1, 1),
        "empty_middle_level": (gap_levels, gap_rows, [8, 1, 15, 4], ASSIGN_LIMIT, ASSIGN_TOPK),
        "point_on_face": ([torch.cat((cells(4, .5), on_face)), cells(2, 1.0)], [gt_row(1.0, 1.0, 1.0, 1.0, 1.0, 1.0)], [13],
                          ASSIGN_LIMIT, ASSIGN_TOPK),
    }


def run_assign(head_mod):
    """the reference's FCAF3DAssigner.assign on scenes of yaw-0 boxes.  Per scene: the level point arrays, the box rows, their
    labels, (limit, topk), the labels of all rows (int16) and, for the rows with label >= 0 in ascending order, the box target
    [P, 7] and the centerness target [P]; the box of a row is told by its label.
    Two things stand in for what is absent.  rotation_3d_in_axis (mmdet3d) is the identity, asserted to be called with zero
    angles only: exact for any convention of that function, so the convention stays UNPINNED by this fixture.  torch.sqrt is
    numpy's correctly rounded one during the run (a torch primitive, not reference code): the CPU's vector library is within
    one ulp but which values it misses depends on the processor."""
    from unittest import mock
    head_mod.rotation_3d_in_axis = rotation_stand_in
    out, names = {}, []
    for name, (levels, rows, labels, limit, topk) in assign_scenes().items():
        assert len(set(labels)) == len(labels) and all(r[6] == 0.0 for r in rows)
        gt = GTStandIn(rows)
        with mock.patch.object(torch, "sqrt", ieee_sqrt):
            ctr, box_t, lab = head_mod.FCAF3DAssigner(limit, topk, len(levels)).assign(levels, gt, torch.tensor(labels))
        pos = torch.nonzero(lab >= 0).view(-1)
        assert ctr.dtype == box_t.dtype == torch.float32 and len(lab) == sum(len(p) for p in levels)
        for i, p in enumerate(levels):
            out[f"assign.{name}.level{i}"] = p.numpy()
        out[f"assign.{name}.boxes"] = gt.tensor.numpy()
        out[f"assign.{name}.gt_labels"] = np.array(labels, dtype=np.int16)
        out[f"assign.{name}.limit_topk"] = np.array([limit, topk], dtype=np.int32)
        out[f"assign.{name}.labels"] = lab.numpy().astype(np.int16)
        out[f"assign.{name}.pos_box_target"] = box_t[pos].numpy()
        out[f"assign.{name}.pos_centerness"] = ctr[pos].numpy()
        names.append(name)
        print(f"  assign {name}: levels {[len(p) for p in levels]}, {len(rows)} boxes, limit {limit}, topk {topk}: "
              f"{len(pos)} positive rows, labels {sorted(set(lab[pos].tolist()))}")
    out["assign.names"] = np.array(names)
    # the premises the scenes are for, on the reference's own output
    count = lambda name, label: int((out[f"assign.{name}.labels"] == label).sum())
    assert 0 < count("lattice", 3) and 0 < count("lattice", 7) and count("lattice", 2) == 0 and count("lattice", 5) == 0
    lattice = assign_scenes()["lattice"]                     # ties at the k-th value: alone, box 0 keeps fewer than topk rows
    with mock.patch.object(torch, "sqrt", ieee_sqrt):
        alone = head_mod.FCAF3DAssigner(ASSIGN_LIMIT, ASSIGN_TOPK, 4).assign(lattice[0], GTStandIn(lattice[1][:1]), torch.tensor([3]))[2]
    assert 0 < int((alone >= 0).sum()) < ASSIGN_TOPK
    assert all(count("best_level", label) > 0 for label in (1, 2, 3))
    assert count("few_points", 4) == 4 and count("few_points_one_level", 4) == 6
    assert count("point_on_face", 13) == 9 and (out["assign.point_on_face.labels"][64:68] == -1).all()
    assert 0 < (out["assign.random_top1_limit1.labels"] >= 0).sum() <= 5 < (out["assign.random.labels"] >= 0).sum()
    assert (out["assign.empty_middle_level.labels"] >= 0).any()
    return out


def loss_stand_ins(record):
    """the three mmdet losses the shipped configuration names, written out in float64 numpy (mmdet is absent): sigmoid focal
    loss (gamma 2, alpha 0.25), sigmoid cross entropy, axis-aligned IoU3D loss -- each sum / avg_factor.  Every call's
    arguments go to `record`.  The formulas are NOT what this fixture pins; which rows, targets, weights and normalisers the
    reference hands them is."""
    as64 = lambda t: t.detach().double().numpy()
    softplus_neg_abs = lambda x: np.log1p(np.exp(-np.abs(x)))

    def focal(pred, labels, avg_factor=None):
        x, lab = as64(pred), labels.numpy()
        t = np.zeros_like(x)
        hit = (lab >= 0) & (lab < x.shape[1])
        t[np.nonzero(hit)[0], lab[hit]] = 1.0
        p = 1.0 / (1.0 + np.exp(-x))
        pt = (1 - p) * t + p * (1 - t)
        loss = (np.maximum(x, 0) - x * t + softplus_neg_abs(x)) * (0.25 * t + 0.75 * (1 - t)) * pt ** 2.0
        record.append(dict(cls_labels=lab.astype(np.int16), cls_avg_factor=np.float64(avg_factor)))
        return torch.tensor(loss.sum() / float(avg_factor), dtype=torch.float64)

    def bce(pred, target, avg_factor=None):
        x, t = as64(pred), as64(target)
        assert x.shape == t.shape
        record[-1].update(ctr_logit=x[:, 0], ctr_target=target.numpy()[:, 0], ctr_avg_factor=np.float64(avg_factor))
        return torch.tensor((np.maximum(x, 0) - x * t + softplus_neg_abs(x)).sum() / float(avg_factor), dtype=torch.float64)

    def iou3d(pred, target, weight=None, avg_factor=None):
        a, b, w = as64(pred), as64(target), as64(weight)
        ov = np.clip(np.minimum(a[:, :3] + a[:, 3:6] / 2, b[:, :3] + b[:, 3:6] / 2)
                     - np.maximum(a[:, :3] - a[:, 3:6] / 2, b[:, :3] - b[:, 3:6] / 2), 0, None).prod(1)
        iou = ov / np.clip(a[:, 3:6].prod(1) + b[:, 3:6].prod(1) - ov, 1e-8, None)
        record[-1].update(box_pred=a, box_target=target.numpy(), box_weight=weight.numpy(), box_avg_factor=np.float64(avg_factor))
        return torch.tensor(((1 - iou) * w).sum() / float(avg_factor), dtype=torch.float64)

    return focal, bce, iou3d


def loss_scenes():
    """two scenes of four levels (6^3 / 4^3 / 2^3 / 1 cell centres) for one call of loss(): per scene the head outputs of every
    level (float64 values on a 1/16 grid, 6 regression outputs), the points, the box rows and labels.  The second scene's only
    box lies far from every point: no positive row"""
    rng = np.random.RandomState(21)
    pts = [cells(n, s) for n, s in ((6, .16), (4, .24), (2, .48), (1, .96))]
    grid = lambda a: torch.from_numpy(np.round(a * 16) / 16)
    scenes = []
    for rows, labels in (([gt_row(.45, .50, .42, .70, .62, .66), gt_row(.30, .62, .55, .28, .30, .26), gt_row(.66, .30, .30, .40, .34, .44)],
                          [5, 16, 0]), ([gt_row(4.0, 4.0, 4.0, .5, .5, .5)], [9])):
        scenes.append(dict(centerness=[grid(rng.randn(len(p), 1)) for p in pts],
                           bbox_pred=[grid(rng.uniform(.05, .45, (len(p), 6))) for p in pts],
                           cls_score=[grid(rng.randn(len(p), 18) * 2 - 3) for p in pts], points=pts, rows=rows, labels=labels))
    return scenes


def run_head_loss(head_mod):
    """the reference's own FCAF3DHead.loss (:142-214) on loss_scenes(): the head is built by __new__ with the reference's
    assigner and loss_stand_ins().  Stored: the inputs, the three losses (float64) and what the reference handed each stand-in
    per scene -- the labels of all rows, the positive rows' logits, targets, decoded boxes and weights, and the avg_factors.
    The head outputs are float64 (values exact in float32), the points float32: the assignment runs in float32 like run_assign
    (same two stand-ins), everything after it in float64."""
    from unittest import mock
    head_mod.rotation_3d_in_axis = rotation_stand_in
    scenes, record, out = loss_scenes(), [], {}
    h = head_mod.FCAF3DHead.__new__(head_mod.FCAF3DHead)
    h.yaw_parametrization = "fcaf3d"
    h.assigner = head_mod.FCAF3DAssigner(ASSIGN_LIMIT, ASSIGN_TOPK, 4)
    h.loss_cls, h.loss_centerness, h.loss_bbox = loss_stand_ins(record)
    per_level = lambda key: [[sc[key][l] for sc in scenes] for l in range(4)]
    with mock.patch.object(torch, "sqrt", ieee_sqrt):
        loss = h.loss(per_level("centerness"), per_level("bbox_pred"), per_level("cls_score"), per_level("points"),
                      [GTStandIn(sc["rows"]) for sc in scenes], [torch.tensor(sc["labels"]) for sc in scenes])
    assert len(record) == 2 and "box_pred" in record[0] and "box_pred" not in record[1]      # scene 1 took the else branch
    assert (record[1]["cls_labels"] == -1).all() and record[1]["cls_avg_factor"] == 1.0
    for k in ("loss_centerness", "loss_bbox", "loss_cls"):
        assert loss[k].dtype == torch.float64
        out[f"loss.{k}"] = np.float64(loss[k])
    for s, (sc, rec) in enumerate(zip(scenes, record)):
        for l in range(4):
            out[f"loss.scene{s}.points{l}"] = sc["points"][l].numpy()
            for key in ("centerness", "bbox_pred", "cls_score"):
                out[f"loss.scene{s}.{key}{l}"] = sc[key][l].numpy().astype(np.float32)
                assert (out[f"loss.scene{s}.{key}{l}"] == sc[key][l].numpy()).all()
        out[f"loss.scene{s}.boxes"] = np.array(sc["rows"], dtype=np.float32)
        out[f"loss.scene{s}.gt_labels"] = np.array(sc["labels"], dtype=np.int16)
        for key, value in rec.items():
            out[f"loss.scene{s}.handed.{key}"] = value
    print(f"  loss: {({k: float(v) for k, v in loss.items()})}; positive rows per scene "
          f"{[int((r['cls_labels'] >= 0).sum()) for r in record]}, avg_factors "
          f"{[(float(r['cls_avg_factor']), float(r.get('box_avg_factor', 'nan'))) for r in record]}")
    return out


def run_targets(head_mod):
    out = dict(run_assign(head_mod), **run_head_loss(head_mod))
    path = os.path.join(HERE, "fcaf3d_assign.npz")
    save_stable(path, out)
    print(f"fcaf3d_assign.npz written ({os.path.getsize(path)} bytes)")


def run_point_transforms(tr):
    """a8 train path: the point helpers of fcaf3d_transforms.py:152-200 on seeded points"""
    g = torch.Generator().manual_seed(9)
    pts = torch.randn(64, 11, generator=g)
    out = dict(points=pts.numpy())
    out["rot"] = tr.rotate_points(pts.clone(), 0.0731).numpy()
    out["flip_h"] = tr.flip_points(pts.clone(), "horizontal").numpy()
    out["flip_v"] = tr.flip_points(pts.clone(), "vertical").numpy()
    out["scale"] = tr.scale_points(pts.clone(), 1.0625).numpy()
    out["trans"] = tr.translate_points(pts.clone(), np.array([0.1, -0.05, 0.2], dtype=np.float32)).numpy()
    np.random.seed(21)
    mask = tr.sample_points(torch.zeros(1000, 3), max_points=123)
    out["sample_mask_seed21"] = mask.numpy()
    np.savez_compressed(os.path.join(HERE, "point_transforms.npz"), **out)
    print("point_transforms.npz written")


def run_atlas3d():
    """dense 3D U-Net + TSDF head of the reference on a small random volume: parameters, input and outputs"""
    b3, ah = R.load_reference_atlas3d()
    out = {}
    for tag, cond in (("plain", False), ("cond", True)):
        torch.manual_seed(11 + cond)
        net = b3.AtlasBackbone3D(channels=[2, 4, 8, 16], layers_down=[1, 2, 1, 1], layers_up=[1, 2, 1], drop=0.0,
                                 zero_init_residual=False, cond_proj=cond, norm="BN").eval()
        head = ah.AtlasTSDFHead(input_channels=[2, 4, 8], n_scales=3, voxel_size=0.04, label_smoothing=1.05,
                                sparse_threshold=[0.99, 0.99]).eval()
        with torch.no_grad():
            for m in net.modules():                       # non-trivial running statistics
                if isinstance(m, torch.nn.BatchNorm3d):
                    m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
                    m.weight.normal_(1, 0.2); m.bias.normal_(0, 0.2)
            x = torch.randn(1, 2, 16, 16, 8)
            x[:, :, :5] = 0                               # an unobserved slab (exercises the conditional projection)
            feats = net(x)
            tsdf, _ = head(feats)                          # decoder features are already coarse -> fine
        out[f"{tag}_x"] = x.numpy()
        for k, v in net.state_dict().items():
            out[f"{tag}_net.{k}"] = v.numpy()
        for k, v in head.state_dict().items():
            out[f"{tag}_head.{k}"] = v.numpy()
        for i, f in enumerate(feats):
            out[f"{tag}_feat{i}"] = f.numpy()
        for k, v in tsdf.items():
            out[f"{tag}_{k}"] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "atlas3d.npz"), **out)
    print("atlas3d.npz", {k: v.shape for k, v in out.items() if "feat" in k or "tsdf" in k})


CFG_2D = dict(
    fpn=dict(bottom_up_cfg=dict(input_channels=3, norm="BN", depth=50, out_features=["res2", "res3", "res4", "res5"], num_groups=1,
                                width_per_group=64, stride_in_1x1=True, res5_dilation=1, res2_out_channels=256,
                                stem_out_channels=64, freeze_at=2),
             in_features=["res2", "res3", "res4", "res5"], out_channels=256, norm="BN", fuse_type="sum"),
    head=dict(feature_strides={"p2": 4, "p3": 8, "p4": 16, "p5": 32, "p6": 64},
              feature_channels={"p2": 256, "p3": 256, "p4": 256, "p5": 256, "p6": 256}, output_dim=32, output_stride=4, norm="BN"))


def run_backbone2d():
    """the reference's ResNet-50 FPN + AtlasFPNFeature (the shipped configuration) on a small image; the weights are a
    function of their state-dict key (tests/helpers.py), so only input and outputs are kept"""
    sys.path.insert(0, os.path.dirname(HERE))
    from helpers import fill_state_deterministic
    fpn_m, b2_m = R.load_reference_2d()
    fpn = fill_state_deterministic(fpn_m.FPNDetectron(**CFG_2D["fpn"])).eval()
    head = fill_state_deterministic(b2_m.AtlasFPNFeature(**CFG_2D["head"])).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 96, generator=g) * 40.0
    with torch.no_grad():
        pyr = fpn(x)
        y = head(pyr)
    out = dict(x=x.numpy(), y=y.numpy(), p2=pyr["p2"].numpy(), p6=pyr["p6"].numpy(),
               fpn_keys=np.array(sorted(fpn.state_dict())), head_keys=np.array(sorted(head.state_dict())))
    np.savez_compressed(os.path.join(HERE, "backbone2d.npz"), **out)
    print("backbone2d.npz", y.shape, {k: tuple(v.shape) for k, v in pyr.items()})


def main():
    torch.set_num_threads(8)
    rm, head, tr, ts = R.load_reference()
    run_scene(rm, tr, "tiny", scene("tiny", seed=0))
    run_scene(rm, tr, "tiny_boxes_origin", scene("tiny", seed=1, boxes=3, origin=(-0.52, 0.24, -0.12)), thr=0.03)
    # plumbing-like aspect (stride 1, more channels), kept small enough for a fixture
    run_scene(rm, tr, "mini_p", scene((2, 16, 32, 32, (48, 48, 32), 1), seed=2))
    # edge: view 0 looks away from the grid (no kept sample -> the reference returns None and skips it)
    sc = scene("tiny", seed=4, V=2)
    P = sc["projection"]
    P[0, 0, :, :3] = -P[0, 0, :, :3]            # mirror the camera through its centre: every ray leaves the grid
    run_scene(rm, tr, "edge_empty_view", sc)
    run_edge_scenes(rm, tr)
    run_quirk_scene(rm, "edge_single_sample", quirk_neus_scene(0))
    run_quirk_scene(rm, "edge_single_sample_v1", quirk_neus_scene(1))
    run_quirk_scene(rm, "edge_single_sample_depth", quirk_depth_scene())
    run_quirk_single_view(rm, "edge_single_sample_only", quirk_neus_scene(0))
    run_depth_edges(rm)
    run_decode(head)
    run_targets(head)
    run_point_transforms(tr)
    run_atlas3d()
    run_backbone2d()


if __name__ == "__main__" and "--backbone2d" in sys.argv:
    run_backbone2d()
    sys.exit(0)

if __name__ == "__main__" and "--quirks" in sys.argv:
    _rm = R.load_reference()[0]
    run_quirk_scene(_rm, "edge_single_sample", quirk_neus_scene(0))
    run_quirk_scene(_rm, "edge_single_sample_v1", quirk_neus_scene(1))
    run_quirk_scene(_rm, "edge_single_sample_depth", quirk_depth_scene())
    run_quirk_single_view(_rm, "edge_single_sample_only", quirk_neus_scene(0))
    sys.exit(0)

if __name__ == "__main__" and "--edges" in sys.argv:
    _rm, _, _tr, _ = R.load_reference()
    run_edge_scenes(_rm, _tr)
    sys.exit(0)

if __name__ == "__main__" and "--depth-edges" in sys.argv:
    run_depth_edges(R.load_reference()[0])
    sys.exit(0)

if __name__ == "__main__" and "--targets" in sys.argv:
    run_targets(R.load_reference()[1])
    sys.exit(0)

if __name__ == "__main__" and "--atlas3d" in sys.argv:
    run_atlas3d()
    sys.exit(0)

if __name__ == "__main__":
    main()
