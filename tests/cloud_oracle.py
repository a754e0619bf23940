"""Host oracle of cnrma_amd.cloud (csrc/cloud.hip): numpy fp64, plus scipy's cKDTree where brute force is too large.  Every formula
is the prescribed one of include/cnrma.h (a15), so the device results are compared bit for bit."""
import numpy as np

BRUTE_PAIRS = 4_000_000
KEY_LIMIT = 1 << 21


def voxel_keys(points, vs, dtype=np.float64):
    """k [N,3] = floor((p - (lo - vs / 2)) / vs) computed in `dtype` (float64 is the contract; float32 shows what a single-precision
    key path would give)"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lo = p.min(axis=0)
    v = dtype(vs)
    org = lo.astype(dtype) - dtype(0.5) * v
    return np.floor((p.astype(dtype) - org) / v).astype(np.int64)


def down_sample(points, vs):
    """-> (points [V,3] float32 in ascending (kx, ky, kz), counts [V] int32).  Sums in fp64 in ascending input index."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32)
    if not np.isfinite(p).all():
        raise ValueError("non-finite coordinate")
    k = voxel_keys(p, vs)
    if (k >= KEY_LIMIT).any():
        raise ValueError("voxel size too small")
    key = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    uniq, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    sums = np.zeros((len(uniq), 3), np.float64)
    np.add.at(sums, inv.reshape(-1), p.astype(np.float64))       # unbuffered: one addition per row, in index order
    return (sums / counts[:, None].astype(np.float64)).astype(np.float32), counts.astype(np.int32)


def _d2(q, t):
    """the prescribed arithmetic: (dx*dx + dy*dy) + dz*dz in fp64; q [..,3], t [..,3] broadcast"""
    d = q.astype(np.float64) - t.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_brute(queries, targets):
    q = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(targets, dtype=np.float32).reshape(-1, 3)
    if len(t) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, np.int32)
    dist, idx = np.empty(len(q), np.float64), np.empty(len(q), np.int32)
    step = max(1, BRUTE_PAIRS // len(t))
    for s in range(0, len(q), step):
        d2 = _d2(q[s:s + step, None, :], t[None, :, :])
        i = d2.argmin(axis=1)                                     # the first minimum = the lowest index
        idx[s:s + step] = i
        dist[s:s + step] = np.sqrt(d2[np.arange(len(i)), i])
    return dist, idx


def nearest_tree(queries, targets):
    """cKDTree proposes the distance; all targets within d (1 + 1e-12) are re-scored with the prescribed arithmetic and the
    lexicographic minimum (d2, index) is taken"""
    from scipy.spatial import cKDTree
    q = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(targets, dtype=np.float32).reshape(-1, 3)
    if len(t) == 0:
        return np.full(len(q), np.inf), np.full(len(q), -1, np.int32)
    tree = cKDTree(t.astype(np.float64))
    d, _ = tree.query(q.astype(np.float64), k=1)
    cand = tree.query_ball_point(q.astype(np.float64), d * (1.0 + 1e-12) + 1e-300)
    dist, idx = np.empty(len(q), np.float64), np.empty(len(q), np.int32)
    for j, c in enumerate(cand):
        c = np.sort(np.asarray(c, dtype=np.int64))
        d2 = _d2(q[j][None, :], t[c])
        b = d2.argmin()
        idx[j] = c[b]
        dist[j] = np.sqrt(d2[b])
    return dist, idx


def nearest(queries, targets):
    if len(queries) * len(targets) <= BRUTE_PAIRS:
        return nearest_brute(queries, targets)
    return nearest_tree(queries, targets)


def eval_mesh(pred, gt, threshold=.05, down_sample_size=.02):
    """the reference's eval_mesh on arrays -> (metrics, counts): counts = (#pred below threshold, #pred, #gt below, #gt)"""
    p = np.asarray(pred, dtype=np.float32).reshape(-1, 3)
    g = np.asarray(gt, dtype=np.float32).reshape(-1, 3)
    if down_sample_size:
        p, g = down_sample(p, down_sample_size)[0], down_sample(g, down_sample_size)[0]
    nan = float("nan")
    if len(p) == 0 or len(g) == 0:
        return {k: nan for k in ("dist1", "dist2", "prec", "recal", "fscore")}, (0, len(p), 0, len(g))
    d_pg, d_gp = nearest(p, g)[0], nearest(g, p)[0]
    prec, recal = float(np.mean((d_pg < threshold).astype("float"))), float(np.mean((d_gp < threshold).astype("float")))
    m = {"dist1": float(np.mean(d_pg)), "dist2": float(np.mean(d_gp)), "prec": prec, "recal": recal,
         "fscore": 2 * prec * recal / (prec + recal) if prec + recal > 0 else nan}
    return m, (int((d_pg < threshold).sum()), len(p), int((d_gp < threshold).sum()), len(g))
