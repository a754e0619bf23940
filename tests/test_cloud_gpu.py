"""GPU tests of the device mesh evaluation (cnrma_amd.cloud / csrc/cloud.hip) against the host oracle tests/cloud_oracle.py.

"Equals the oracle" means throughout: voxel counts, out_count and idx equal as integers, points bit-equal in float32, dist
bit-equal in float64 -- every formula is prescribed and un-fused, and the nearest neighbour does not depend on the search grid."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
import torch

import cloud_oracle as CO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY_F, CANARY_I, CANARY_D = -12345.5, -77, -4321.25
PAD = 8


def _dev(a, device, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()


def _raw_down(p, vs, device, out_cap=None, n_live=None, count=True):
    """the C ABI with canary-padded outputs -> info [4], out_points, out_count (whole buffers, on the host)"""
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr, stream
    n = len(p)
    pts = _dev(np.asarray(p, np.float32).reshape(-1, 3), device)
    out_cap = n if out_cap is None else out_cap
    out = torch.full((out_cap + PAD, 3), CANARY_F, dtype=torch.float32, device=device)
    cnt = torch.full((out_cap + PAD,), CANARY_I, dtype=torch.int32, device=device)
    info = torch.full((4 + PAD,), CANARY_I, dtype=torch.int32, device=device)
    nbytes = _lib.load().cnrma_cloud_downsample_workspace_bytes(n)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    n_dev = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=device)
    call("cnrma_cloud_voxel_downsample_f32", ptr(pts) if n else None, n, ptr(n_dev), float(vs), ptr(ws), nbytes, ptr(out),
         ptr(cnt) if count else None, out_cap, ptr(info), stream())
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert (info[4:] == CANARY_I).all()
    return info[:4], out.cpu().numpy(), cnt.cpu().numpy()


def _assert_down_equals_oracle(p, vs, device, **kw):
    exp_p, exp_c = CO.down_sample(p if kw.get("n_live") is None else p[:kw["n_live"]], vs)
    info, out, cnt = _raw_down(p, vs, device, **kw)
    v = len(exp_p)
    assert info.tolist() == [v, 0, 0, 0]
    assert np.array_equal(cnt[:v], exp_c)
    assert np.array_equal(out[:v].view(np.uint32), exp_p.view(np.uint32))
    assert (out[v:] == CANARY_F).all() and (cnt[v:] == CANARY_I).all()
    return exp_p, exp_c


def _raw_nn(q, t, device, cell=0.04, nq_live=None, nt_live=None):
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr, stream
    nq, nt = len(q), len(t)
    qd, td = _dev(np.asarray(q, np.float32).reshape(-1, 3), device), _dev(np.asarray(t, np.float32).reshape(-1, 3), device)
    nbytes = _lib.load().cnrma_cloud_nn_workspace_bytes(nt)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dist = torch.full((nq + PAD,), CANARY_D, dtype=torch.float64, device=device)
    idx = torch.full((nq + PAD,), CANARY_I, dtype=torch.int32, device=device)
    nq_dev = None if nq_live is None else torch.tensor([nq_live], dtype=torch.int32, device=device)
    nt_dev = None if nt_live is None else torch.tensor([nt_live], dtype=torch.int32, device=device)
    call("cnrma_cloud_nn_build_f32", ptr(td) if nt else None, nt, ptr(nt_dev), float(cell), ptr(ws), nbytes, stream())
    call("cnrma_cloud_nn_query_f32", ptr(qd) if nq else None, nq, ptr(nq_dev), nt, ptr(ws), ptr(dist), ptr(idx), None, stream())
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy()


def _assert_nn_equals_oracle(q, t, device, cell=0.04, nq_live=None, nt_live=None, oracle=CO.nearest):
    q, t = np.asarray(q, np.float32).reshape(-1, 3), np.asarray(t, np.float32).reshape(-1, 3)
    lq, lt = len(q) if nq_live is None else nq_live, len(t) if nt_live is None else nt_live
    exp_d, exp_i = oracle(q[:lq], t[:lt])
    dist, idx = _raw_nn(q, t, device, cell, nq_live, nt_live)
    assert np.array_equal(idx[:lq], exp_i)
    assert np.array_equal(dist[:lq].view(np.uint64), exp_d.view(np.uint64))
    assert (dist[lq:] == CANARY_D).all() and (idx[lq:] == CANARY_I).all()
    return dist[:lq], idx[:lq]


# ---------------------------------------------------------------------------------------------------------------
# voxel down-sample
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100_003])
def test_down_sample_sizes(device, n):
    p = np.random.default_rng(n).uniform(0, 4, (n, 3)).astype(np.float32)
    exp_p, _ = _assert_down_equals_oracle(p, 0.02, device)
    if n > 1000:
        assert 1000 < len(exp_p) < n                              # both crowded and single voxels


def test_down_sample_identical_points(device):
    p = np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (1000, 1))
    _, exp_c = _assert_down_equals_oracle(p, 0.02, device)
    assert exp_c.tolist() == [1000]


def test_down_sample_points_on_voxel_faces(device):
    """coordinates lo + j vs / 2: every other one sits exactly on a face of the voxel grid (org = lo - vs / 2)"""
    rng = np.random.default_rng(7)
    vs = 0.02
    j = rng.integers(0, 40, (5000, 3))
    j[0] = 0
    p = (np.float32(-0.25) + j.astype(np.float64) * (vs / 2)).astype(np.float32)
    _assert_down_equals_oracle(p, vs, device)
    p = (j.astype(np.float64) * 0.25).astype(np.float32)         # exactly representable faces: vs = 0.5, org = -0.25
    _assert_down_equals_oracle(p, 0.5, device)


def test_down_sample_negative_coordinates(device):
    p = np.random.default_rng(8).uniform(-3, -1, (5000, 3)).astype(np.float32)
    p[:, 1] += 2.0                                                # y straddles 0
    _assert_down_equals_oracle(p, 0.02, device)


def test_down_sample_membership_is_fp64(device):
    """200 000 points in [1000, 1004)^3: fp32 key arithmetic puts hundreds of points into another voxel (checked here on the host
    first), so a single-precision key path cannot pass"""
    p = (1000.0 + np.random.default_rng(0).uniform(0, 4, (200_000, 3))).astype(np.float32)
    differ = (CO.voxel_keys(p, 0.02, np.float32) != CO.voxel_keys(p, 0.02, np.float64)).any(axis=1).sum()
    assert differ >= 100, differ
    _assert_down_equals_oracle(p, 0.02, device)


def test_down_sample_capacity(device):
    """out_cap below the need: the rows behind it keep the canary, info[0] holds the true count; out_count may be NULL"""
    p = np.random.default_rng(9).uniform(0, 1, (3000, 3)).astype(np.float32)
    exp_p, exp_c = CO.down_sample(p, 0.02)
    cap = len(exp_p) // 2
    info, out, cnt = _raw_down(p, 0.02, device, out_cap=cap)
    assert info.tolist() == [len(exp_p), 0, 0, 0]
    assert np.array_equal(out[:cap].view(np.uint32), exp_p[:cap].view(np.uint32)) and np.array_equal(cnt[:cap], exp_c[:cap])
    assert (out[cap:] == CANARY_F).all() and (cnt[cap:] == CANARY_I).all()
    info, out, cnt = _raw_down(p, 0.02, device, count=False)
    assert info[0] == len(exp_p) and np.array_equal(out[:len(exp_p)].view(np.uint32), exp_p.view(np.uint32))
    assert (cnt == CANARY_I).all()
    info, out, _ = _raw_down(p, 0.02, device, out_cap=0)
    assert info[0] == len(exp_p) and (out == CANARY_F).all()


def test_down_sample_flags(device):
    from cnrma_amd import cloud
    p = np.random.default_rng(10).uniform(0, 1, (500, 3)).astype(np.float32)
    wide = p.copy()
    wide[7, 1] = 0.02 * (1 << 21) + 10.0                          # extent / vs above 2^21
    info, out, cnt = _raw_down(wide, 0.02, device)
    assert info.tolist() == [0, cloud.VOXEL_TOO_SMALL, 0, 0] and (out == CANARY_F).all() and (cnt == CANARY_I).all()
    with pytest.raises(ValueError, match="too small"):
        cloud.voxel_down_sample(_dev(wide, device), 0.02)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[311, 2] = bad
        info, out, _ = _raw_down(q, 0.02, device)
        assert info[1] & cloud.NONFINITE and info[0] == 0 and (out == CANARY_F).all()
    with pytest.raises(ValueError, match="NaN"):
        cloud.voxel_down_sample(_dev(q, device), 0.02)
    with pytest.raises(ValueError):
        cloud.eval_mesh(_dev(q, device), _dev(p, device))


@pytest.mark.parametrize("live", [0, 1, 200, 299])
def test_down_sample_device_row_count(device, live):
    """n_dev below n_cap: the dead rows are NaN and must not be read"""
    p = np.random.default_rng(11).uniform(0, 0.5, (300, 3)).astype(np.float32)
    p[live:] = np.nan
    _assert_down_equals_oracle(p, 0.02, device, n_live=live)


def test_voxel_down_sample_wrapper(device):
    from cnrma_amd import cloud
    p = np.random.default_rng(12).uniform(0, 1, (4000, 3)).astype(np.float32)
    out, n_dev = cloud.voxel_down_sample(_dev(p, device), 0.02)
    exp_p, _ = CO.down_sample(p, 0.02)
    assert out.shape == (4000, 3) and n_dev.dtype == torch.int32 and n_dev.is_cuda
    n = int(n_dev.cpu()[0])
    assert n == len(exp_p) and np.array_equal(out[:n].cpu().numpy().view(np.uint32), exp_p.view(np.uint32))
    out, n_dev = cloud.voxel_down_sample(p, 0.02)                 # a numpy array goes to the current device
    assert int(n_dev.cpu()[0]) == n


# ---------------------------------------------------------------------------------------------------------------
# nearest neighbour
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,nt", [(1, 1), (64, 1), (1, 64), (63, 65), (65, 63), (1000, 1000)])
def test_nearest_sizes(device, nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    _assert_nn_equals_oracle(rng.uniform(0, 1, (nq, 3)), rng.uniform(0, 1, (nt, 3)), device, oracle=CO.nearest_brute)


def test_nearest_large(device):
    rng = np.random.default_rng(21)
    _assert_nn_equals_oracle(rng.uniform(0, 4, (100_003, 3)), rng.uniform(0, 4, (50_021, 3)), device, oracle=CO.nearest_tree)


def test_nearest_exact_ties(device):
    """integer coordinates: every d2 is exact.  Each query sits at a lattice centre whose six +-1 neighbours are all targets, in
    shuffled order and with every row duplicated: idx is the lowest of the twelve"""
    rng = np.random.default_rng(22)
    centres = np.stack(np.meshgrid(np.arange(0, 24, 3), np.arange(0, 24, 3), np.arange(0, 24, 3), indexing="ij"), -1).reshape(-1, 3)
    off = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    t = (centres[:, None, :] + off[None]).reshape(-1, 3)
    t = np.concatenate([t, t])
    t = t[rng.permutation(len(t))].astype(np.float32)
    for cell in (0.7, 1.0, 2.5):
        dist, idx = _assert_nn_equals_oracle(centres.astype(np.float32), t, device, cell=cell, oracle=CO.nearest_brute)
        assert (dist == 1.0).all()
    for c, i in zip(centres[:50], idx[:50]):
        near = np.flatnonzero(np.abs(t - c).sum(axis=1) == 1)
        assert len(near) == 12 and i == near.min()


def test_nearest_queries_equal_targets(device):
    rng = np.random.default_rng(23)
    t = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    t = np.concatenate([t, t[:300]])                              # duplicates: the first one wins
    dist, idx = _assert_nn_equals_oracle(t, t, device, oracle=CO.nearest_brute)
    assert (dist == 0).all() and np.array_equal(idx, np.concatenate([np.arange(700), np.arange(300)]))


def test_nearest_queries_far_outside(device):
    """10 x the extent away along the six axis directions and the eight corners"""
    rng = np.random.default_rng(24)
    t = rng.uniform(0, 1, (2000, 3)).astype(np.float32)
    dirs = [d for d in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
            if np.abs(d).sum() in (1, 3)]
    assert len(dirs) == 14
    q = np.array([0.5 + 10.0 * d + rng.uniform(-0.3, 0.3, 3) for d in dirs for _ in range(4)], np.float32)
    _assert_nn_equals_oracle(q, t, device, cell=0.05, oracle=CO.nearest_brute)


def test_nearest_two_clusters_many_empty_shells(device):
    rng = np.random.default_rng(25)
    a = rng.uniform(0, 0.1, (300, 3))
    t = np.concatenate([a, a[::-1] + [2.0, 0, 0]]).astype(np.float32)       # 50 cells of 0.04 apart
    q = (np.array([1.05, 0.05, 0.05]) + rng.uniform(-0.02, 0.02, (200, 3))).astype(np.float32)
    q[0] = [1.05, 0.05, 0.05]
    _assert_nn_equals_oracle(q, t, device, cell=0.04, oracle=CO.nearest_brute)


def test_nearest_all_targets_in_one_cell(device):
    rng = np.random.default_rng(26)
    t = rng.uniform(0, 0.01, (500, 3)).astype(np.float32)
    q = rng.uniform(-0.1, 0.1, (300, 3)).astype(np.float32)
    _assert_nn_equals_oracle(q, t, device, cell=0.04, oracle=CO.nearest_brute)


@pytest.mark.parametrize("flat", [(1, 2), (0, 2), (2,), (0,)])
def test_nearest_collinear_and_coplanar_targets(device, flat):
    """grid dims of 1 along the flattened axes"""
    rng = np.random.default_rng(27 + len(flat))
    t = rng.uniform(0, 1, (1500, 3)).astype(np.float32)
    t[:, list(flat)] = 0.25
    q = rng.uniform(-0.2, 1.2, (800, 3)).astype(np.float32)
    _assert_nn_equals_oracle(q, t, device, cell=0.03, oracle=CO.nearest_brute)


def test_nearest_cell_cap_enlarges_the_cell(device):
    """10 000 targets in the unit cube and one at (1e4, 1e4, 1e4): 250 000^3 cells of 0.04 are asked for, 2^24 are allowed"""
    rng = np.random.default_rng(29)
    t = np.concatenate([rng.uniform(0, 1, (10_000, 3)), [[1e4, 1e4, 1e4]]]).astype(np.float32)
    q = np.concatenate([rng.uniform(0, 1, (300, 3)), rng.uniform(4000, 6000, (50, 3)), [[9999, 9999, 9999]]]).astype(np.float32)
    _, idx = _assert_nn_equals_oracle(q, t, device, cell=0.04, oracle=CO.nearest_brute)
    assert idx[-1] == 10_000


def test_nearest_points_on_cell_faces(device):
    """targets and queries at origin + j * cell exactly (cell 0.25, coordinates multiples of 0.25): the stopping bound's margin"""
    rng = np.random.default_rng(30)
    t = (rng.integers(0, 24, (3000, 3)) * 0.25).astype(np.float32)
    t[0] = 0
    q = (rng.integers(-4, 28, (2000, 3)) * 0.25).astype(np.float32)
    _assert_nn_equals_oracle(q, t, device, cell=0.25, oracle=CO.nearest_brute)
    t2 = (np.float32(0.1) + rng.integers(0, 50, (3000, 3)).astype(np.float32) * np.float32(0.04)).astype(np.float32)
    q2 = (np.float32(0.1) + rng.integers(0, 50, (2000, 3)).astype(np.float32) * np.float32(0.04)).astype(np.float32)
    _assert_nn_equals_oracle(q2, t2, device, cell=0.04, oracle=CO.nearest_brute)


def test_nearest_does_not_depend_on_the_cell(device):
    rng = np.random.default_rng(31)
    q, t = rng.uniform(0, 2, (5000, 3)).astype(np.float32), rng.uniform(0, 2, (4000, 3)).astype(np.float32)
    ref = _raw_nn(q, t, device, cell=0.04)
    for cell in (0.013, 0.3, 50.0):
        got = _raw_nn(q, t, device, cell=cell)
        assert np.array_equal(got[0].view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(got[1], ref[1])
    exp_d, exp_i = CO.nearest(q, t)
    assert np.array_equal(ref[1][:5000], exp_i) and np.array_equal(ref[0][:5000].view(np.uint64), exp_d.view(np.uint64))


def test_nearest_without_live_targets(device):
    q = np.random.default_rng(32).uniform(0, 1, (70, 3)).astype(np.float32)
    dist, idx = _raw_nn(q, np.zeros((0, 3), np.float32), device)
    assert np.isposinf(dist[:70]).all() and (idx[:70] == -1).all()
    t = np.full((10, 3), np.nan, np.float32)                      # capacity 10, none live, the dead rows NaN
    dist, idx = _raw_nn(q, t, device, nt_live=0)
    assert np.isposinf(dist[:70]).all() and (idx[:70] == -1).all()


@pytest.mark.parametrize("nq_live,nt_live", [(0, 500), (1, 1), (130, 77), (299, 499)])
def test_nearest_device_row_counts(device, nq_live, nt_live):
    rng = np.random.default_rng(33)
    q, t = rng.uniform(0, 1, (300, 3)).astype(np.float32), rng.uniform(0, 1, (500, 3)).astype(np.float32)
    q[nq_live:] = np.nan
    t[nt_live:] = np.nan
    _assert_nn_equals_oracle(q, t, device, nq_live=nq_live, nt_live=nt_live, oracle=CO.nearest_brute)


def test_nearest_wrapper(device):
    from cnrma_amd import cloud
    rng = np.random.default_rng(34)
    q, t = rng.uniform(0, 1, (900, 3)).astype(np.float32), rng.uniform(0, 1, (800, 3)).astype(np.float32)
    exp_d, exp_i = CO.nearest(q, t)
    stats = torch.zeros(2, dtype=torch.int64, device=device)
    for kw in ({}, {"cell": 0.11}, {"stats": stats}):
        dist, idx = cloud.nearest(_dev(q, device), _dev(t, device), **kw)
        assert dist.dtype == torch.float64 and idx.dtype == torch.int32
        assert np.array_equal(idx.cpu().numpy(), exp_i) and np.array_equal(dist.cpu().numpy().view(np.uint64), exp_d.view(np.uint64))
    shells, cands = stats.cpu().tolist()
    assert shells >= 900 and cands >= 900


# ---------------------------------------------------------------------------------------------------------------
# eval_mesh
# ---------------------------------------------------------------------------------------------------------------
def test_eval_mesh_cloud_against_itself(device):
    from cnrma_amd import cloud
    p = np.random.default_rng(40).uniform(0, 2, (5000, 3)).astype(np.float32)
    for ds in (.02, 0):
        m = cloud.eval_mesh(_dev(p, device), _dev(p, device), down_sample=ds)
        assert m == {"dist1": 0.0, "dist2": 0.0, "prec": 1.0, "recal": 1.0, "fscore": 1.0}
        assert all(type(v) is float for v in m.values())


def test_eval_mesh_threshold_is_strict(device):
    """an integer lattice against itself shifted by exactly 0.5: every distance equals the threshold"""
    from cnrma_amd import cloud
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    m = cloud.eval_mesh(g, g + np.array([0.5, 0, 0], np.float32), threshold=0.5, down_sample=0)
    assert m["dist1"] == 0.5 and m["dist2"] == 0.5 and m["prec"] == 0.0 and m["recal"] == 0.0 and np.isnan(m["fscore"])
    m = cloud.eval_mesh(g, g + np.array([0.5, 0, 0], np.float32), threshold=np.nextafter(0.5, 1.0), down_sample=0)
    assert m["prec"] == 1.0 and m["recal"] == 1.0 and m["fscore"] == 1.0


def test_eval_mesh_random_pair_at_the_defaults(device):
    from cnrma_amd import cloud
    rng = np.random.default_rng(41)
    gt = rng.uniform(0, 1.5, (20_000, 3)).astype(np.float32)
    pred = (gt[:16_000] + rng.normal(0, 0.03, (16_000, 3))).astype(np.float32)
    pred = np.concatenate([pred, rng.uniform(0, 1.5, (4000, 3)).astype(np.float32)])
    exp, (cp, n_p, cg, n_g) = CO.eval_mesh(pred, gt)
    r = cloud.eval_mesh_raw(_dev(pred, device), _dev(gt, device))
    assert (int(r[1]), int(r[2]), int(r[4]), int(r[5])) == (cp, n_p, cg, n_g)
    assert 0 < cp < n_p and 0 < cg < n_g                          # the threshold separates
    got = cloud.eval_mesh(_dev(pred, device), _dev(gt, device))
    assert got["prec"] == exp["prec"] and got["recal"] == exp["recal"]
    for k in ("dist1", "dist2", "fscore"):
        print(k, got[k], exp[k])
        assert abs(got[k] - exp[k]) <= 1e-12 * abs(exp[k])


def test_eval_mesh_empty_prediction(device):
    from cnrma_amd import cloud
    g = np.random.default_rng(42).uniform(0, 1, (100, 3)).astype(np.float32)
    for ds in (.02, 0):
        for a, b in ((np.zeros((0, 3), np.float32), g), (g, np.zeros((0, 3), np.float32))):
            m = cloud.eval_mesh(a, b, down_sample=ds)
            assert sorted(m) == ["dist1", "dist2", "fscore", "prec", "recal"] and all(np.isnan(v) for v in m.values())


def test_eval_mesh_marching_cubes_sphere_against_its_ply(device, tmp_path):
    from cnrma_amd import cloud, mesh
    x = np.stack(np.meshgrid(*[np.arange(24, dtype=np.float32)] * 3, indexing="ij"), -1)
    vol = np.clip((np.linalg.norm(x - 11.5, axis=-1) - 8.0) / 3.0, -1, 1).astype(np.float32)
    m = mesh.marching_cubes(_dev(vol, device), 0.04, (-0.5, 0.25, 1.0))
    assert len(m.vertices) > 500
    path = str(tmp_path / "sphere.ply")
    m.export(path)
    got = cloud.eval_mesh(m, cloud.read_ply_points(path))
    assert got == {"dist1": 0.0, "dist2": 0.0, "prec": 1.0, "recal": 1.0, "fscore": 1.0}


def _write_ply(path, pts):
    with open(path, "wb") as fh:
        fh.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(pts)}\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n".encode("ascii"))
        fh.write(np.asarray(pts, "<f4").tobytes())


def test_evaluate_mesh_cli_on_a_scannet_layout(device, tmp_path):
    """two tiny scenes, one with an axisAlignment file: metrics.json equals the oracle's"""
    spec = importlib.util.spec_from_file_location("evaluate_mesh_cli", os.path.join(ROOT, "post_process", "evaluate_mesh.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    rng = np.random.default_rng(43)
    data, result = tmp_path / "data", tmp_path / "result"
    (data / "meta_data").mkdir(parents=True)
    (data / "meta_data" / "scannetv2_val.txt").write_text("scene0002_00\nscene0001_00\n")
    align = np.array([[0, 1, 0, 0.5], [-1, 0, 0, 1.5], [0, 0, 1, -0.25], [0, 0, 0, 1]], np.float64)
    exp = {}
    for k, scene in enumerate(("scene0001_00", "scene0002_00")):
        (data / "scans" / scene).mkdir(parents=True)
        (result / scene).mkdir(parents=True)
        gt = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
        gt_world = gt
        if k == 0:
            (data / "scans" / scene / (scene + ".txt")).write_text(
                "axisAlignment = " + " ".join(repr(float(v)) for v in align.reshape(-1)) + " \nnumColorFrames = 3\n")
            gt_world = (gt.astype(np.float64) @ align[:3, :3].T + align[:3, 3]).astype(np.float32)
        pred = (gt_world[:2400] + rng.normal(0, 0.03, (2400, 3))).astype(np.float32)
        _write_ply(data / "scans" / scene / (scene + "_vh_clean_2.ply"), gt)
        _write_ply(result / scene / (scene + ".ply"), pred)
        exp[scene] = CO.eval_mesh(pred, gt_world)[0]
    args = types.SimpleNamespace(dataset="scannet", data_path=str(data), result_path=str(result), axis_align=1)
    got = cli.evaluate_meshes(args)
    on_disk = json.load(open(result / "metrics.json"))
    assert got == on_disk and sorted(on_disk) == ["scene0001_00", "scene0002_00"]
    for scene in exp:
        assert list(on_disk[scene]) == ["dist1", "dist2", "prec", "recal", "fscore"]
        assert on_disk[scene]["prec"] == exp[scene]["prec"] and on_disk[scene]["recal"] == exp[scene]["recal"]
        assert 0 < exp[scene]["prec"] < 1
        for k in ("dist1", "dist2", "fscore"):
            assert abs(on_disk[scene][k] - exp[scene][k]) <= 1e-12 * abs(exp[scene][k])
