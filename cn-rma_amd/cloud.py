"""Scoring a reconstructed mesh on the device: voxel down-sample, exact nearest neighbour and the five metrics (csrc/cloud.hip;
reference: post_process/evaluate_mesh.py:29-92, eval_mesh / nn_correspondance, which need Open3D on the host).

    m = eval_mesh(pred, gt)          # {'dist1', 'dist2', 'prec', 'recal', 'fscore'}: Python floats, ONE device->host read

`voxel_down_sample` is Open3D's rule written out (fp64 voxel membership relative to the cloud's minimum minus half a voxel, the
mean of a voxel's points summed in fp64 in input order); the voxels come out in ascending (kx, ky, kz), not in Open3D's hash-map
order, which no metric depends on.  `nearest` is exact: fp64 squared distances in a fixed bracket order, ties to the lowest
target index, independent of the search grid -- so it is checked bit for bit against a brute-force oracle.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

NONFINITE, VOXEL_TOO_SMALL = _lib.CONSTANTS["CNRMA_CLOUD_NONFINITE"], _lib.CONSTANTS["CNRMA_CLOUD_VOXEL_TOO_SMALL"]
_KEYS = ("dist1", "dist2", "prec", "recal", "fscore")


def _points(p, device=None):
    """[N,3] tensor / array / Mesh -> contiguous float32 device tensor"""
    if hasattr(p, "vertices"):
        p = p.vertices
    if not torch.is_tensor(p):
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float32)))
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"a point cloud is [N,3], got shape {tuple(p.shape)}")
    if device is None:
        device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return p.detach().to(device=device, dtype=torch.float32).contiguous()


def _workspace(name, n, dev):
    ws = _lib.scratch(name, n, device=dev)
    if ws.numel() == 0:
        raise _lib.CnrmaError(f"{name}: unsupported row count {n}")
    return ws


def _down_sample(pts, voxel_size, n_dev=None):
    """-> (out [n,3], info [4] int32 on the device); nothing is read back"""
    n = int(pts.shape[0])
    dev = pts.device
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    ws = _workspace("cnrma_cloud_downsample_workspace_bytes", n, dev)
    call("cnrma_cloud_voxel_downsample_f32", ptr(pts) if n else None, n, ptr(n_dev), float(voxel_size), ptr(ws), ws.numel(),
         ptr(out) if n else None, None, n, ptr(info), stream())
    return out, info


def _raise_flags(flags, what):
    if flags & NONFINITE:
        raise ValueError(f"{what}: a coordinate is NaN or infinite")
    if flags & VOXEL_TOO_SMALL:
        raise ValueError(f"{what}: voxel_size is too small for the cloud's extent (more than 2^21 voxels along an axis)")


def voxel_down_sample(points, voxel_size):
    """Open3D's voxel_down_sample -> (points [cap,3] float32, n_dev): the first n_dev[0] rows (a device int32 word) are the voxel
    means in ascending voxel order; cap = len(points).  Raises ValueError on a non-finite coordinate or a voxel size too small
    for the extent (one device->host read of the flags)."""
    _lib.require_gpu()
    if not voxel_size > 0:
        raise ValueError(f"voxel_size must be positive, got {voxel_size}")
    pts = _points(points)
    out, info = _down_sample(pts, voxel_size)
    _raise_flags(_lib.read_ints(info)[1], "voxel_down_sample")
    return out, info[:1]


def nearest(queries, targets, cell=None, *, nq_dev=None, nt_dev=None, stats=None):
    """for every live query its nearest live target -> (dist [nq] float64, idx [nq] int32; +inf / -1 without a live target).
    `cell` is the search grid's cell size (default: a fixed 0.04); it changes the time, never the result.  Rows behind nq_dev are
    not written.  No device->host read."""
    _lib.require_gpu()
    q = _points(queries)
    t = _points(targets, q.device)
    dev = q.device
    nq, nt = int(q.shape[0]), int(t.shape[0])
    cell = 0.04 if cell is None else float(cell)
    if not cell > 0:
        raise ValueError(f"cell must be positive, got {cell}")
    ws = _workspace("cnrma_cloud_nn_workspace_bytes", nt, dev)
    dist = torch.empty(nq, dtype=torch.float64, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    call("cnrma_cloud_nn_build_f32", ptr(t) if nt else None, nt, ptr(nt_dev), cell, ptr(ws), ws.numel(), stream())
    if nq:
        call("cnrma_cloud_nn_query_f32", ptr(q), nq, ptr(nq_dev), nt, ptr(ws), ptr(dist), ptr(idx), ptr(stats), stream())
    return dist, idx


def _score(dist, n_dev, threshold, out3):
    n = int(dist.shape[0])
    ws = _workspace("cnrma_cloud_score_workspace_bytes", n, dist.device)
    call("cnrma_cloud_score_f64", ptr(dist) if n else None, n, ptr(n_dev), float(threshold), ptr(ws), ws.numel(), ptr(out3), stream())


def default_cell(threshold=.05, down_sample=.02):
    """the search cell eval_mesh uses: a fixed function of its arguments (scripts/cloud_probe.py compares the candidates)"""
    return 2.0 * float(down_sample) if down_sample else float(threshold)


def eval_mesh_raw(pred, gt, threshold=.05, down_sample=.02, cell=None):
    """the device half of eval_mesh -> float64 [8] on the host = {sum, count below threshold, rows} of pred -> gt, the same of
    gt -> pred, and the two down-sample flag words; one device->host read"""
    _lib.require_gpu()
    p = _points(pred)
    g = _points(gt, p.device)
    dev = p.device
    block = torch.zeros(8, dtype=torch.float64, device=dev)
    np_dev = ng_dev = None
    if down_sample:
        p, info_p = _down_sample(p, down_sample)
        g, info_g = _down_sample(g, down_sample)
        np_dev, ng_dev = info_p[:1], info_g[:1]
        block[6:7] = info_p[1:2]
        block[7:8] = info_g[1:2]
    cell = default_cell(threshold, down_sample) if cell is None else cell
    d_pg, _ = nearest(p, g, cell, nq_dev=np_dev, nt_dev=ng_dev)
    d_gp, _ = nearest(g, p, cell, nq_dev=ng_dev, nt_dev=np_dev)
    _score(d_pg, np_dev, threshold, block[0:3])
    _score(d_gp, ng_dev, threshold, block[3:6])
    host = torch.empty(8, dtype=torch.float64, pin_memory=True)
    host.copy_(block, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return host.numpy().copy()


def eval_mesh(pred, gt, threshold=.05, down_sample=.02):
    """the reference's eval_mesh (evaluate_mesh.py:29-64) with its swapped names: dist1 = mean distance of the predicted points to
    the ground-truth cloud, dist2 = the other direction, prec / recal = the shares of predicted / ground-truth points nearer than
    `threshold` (strictly), fscore = 2 prec recal / (prec + recal).  pred, gt: [N,3] tensors, arrays or mesh.Mesh (its vertices),
    voxel-down-sampled by `down_sample` first unless that is falsy.  An empty cloud on either side gives five NaN, prec + recal
    == 0 gives fscore NaN, as in the reference."""
    r = eval_mesh_raw(pred, gt, threshold, down_sample)
    _raise_flags(int(r[6]), "eval_mesh: predicted cloud")
    _raise_flags(int(r[7]), "eval_mesh: ground-truth cloud")
    n_p, n_g = r[2], r[5]
    nan = float("nan")
    if n_p == 0 or n_g == 0:
        return {k: nan for k in _KEYS}
    prec, recal = float(r[1] / n_p), float(r[4] / n_g)
    return {"dist1": float(r[0] / n_p), "dist2": float(r[3] / n_g), "prec": prec, "recal": recal,
            "fscore": 2 * prec * recal / (prec + recal) if prec + recal > 0 else nan}


# ---------------------------------------------------------------------------------------------------------------
# PLY vertices (host)
# ---------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_ply_points(path):
    """the vertex positions of a PLY file -> float32 [N,3] (numpy).  ASCII, binary_little_endian and binary_big_endian; the file's
    first element must be `vertex` with scalar properties only, x / y / z float or double -- double coordinates are ROUNDED to
    float32 --, every other scalar property is skipped by its size, later elements (faces) are not read.  That covers ScanNet's
    _vh_clean_2.ply, ARKitScenes' _3dod_mesh.ply, trimesh's export and Mesh.export.  Anything else raises ValueError."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, props, n, seen = None, [], None, 0
        while True:
            raw = fh.readline()
            if not raw:
                raise ValueError(f"{path}: the header has no end_header")
            tok = raw.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "end_header":
                break
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                seen += 1
                if seen == 1:
                    if tok[1] != "vertex":
                        raise ValueError(f"{path}: the first element is `{tok[1]}`, not `vertex`")
                    n = int(tok[2])
            elif tok[0] == "property" and seen == 1:
                if tok[1] == "list":
                    raise ValueError(f"{path}: the vertex element has a list property `{tok[-1]}`")
                if tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unknown property type `{tok[1]}`")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"{path}: unknown format `{fmt}`")
        if n is None:
            raise ValueError(f"{path}: no vertex element")
        kinds = dict(props)
        for a in "xyz":
            if kinds.get(a) not in ("f4", "f8"):
                raise ValueError(f"{path}: vertex property `{a}` is {kinds.get(a, 'missing')}, not float or double")
        if len(kinds) != len(props):
            raise ValueError(f"{path}: duplicate vertex property names")
        if fmt == "ascii":
            rows = [fh.readline().split() for _ in range(n)]
            if any(len(r) < len(props) for r in rows):
                raise ValueError(f"{path}: a vertex line has fewer than {len(props)} values")
            col = {name: k for k, (name, _) in enumerate(props)}
            return np.array([[float(r[col[a]]) for a in "xyz"] for r in rows], dtype=np.float64).reshape(-1, 3).astype(np.float32)
        end = "<" if fmt == "binary_little_endian" else ">"
        dt = np.dtype([(name, end + t) for name, t in props])
        data = np.frombuffer(fh.read(n * dt.itemsize), dtype=dt)
        if len(data) != n:
            raise ValueError(f"{path}: {len(data)} vertices in the file, {n} in the header")
        return np.stack([data[a].astype(np.float32) for a in "xyz"], axis=1).reshape(-1, 3)
