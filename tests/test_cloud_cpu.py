"""Host-side tests of the mesh evaluation: the oracle's two nearest-neighbour paths against each other, the down-sample oracle
against a plain dict-of-lists implementation, the PLY reader, the C-ABI table and the CLI's arguments.  No GPU."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import cloud_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli():
    spec = importlib.util.spec_from_file_location("evaluate_mesh_cli", os.path.join(ROOT, "post_process", "evaluate_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_oracle_paths_agree():
    """brute force and the cKDTree path on 2 000 x 2 000: the same indices, bit-equal distances; and the brute-force distance is
    bit-equal to cKDTree's own"""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    q, t = rng.uniform(0, 1, (2000, 3)).astype(np.float32), rng.uniform(0, 1, (2000, 3)).astype(np.float32)
    db, ib = CO.nearest_brute(q, t)
    dt, it = CO.nearest_tree(q, t)
    assert np.array_equal(ib, it)
    assert np.array_equal(db.view(np.uint64), dt.view(np.uint64))
    dk, ik = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
    assert np.array_equal(ik, ib) and np.array_equal(dk.view(np.uint64), db.view(np.uint64))


def test_oracle_ties_go_to_the_lowest_index():
    t = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 1, 0]], np.float32)
    for fn in (CO.nearest_brute, CO.nearest_tree):
        d, i = fn(np.zeros((1, 3), np.float32), t)
        assert i[0] == 0 and d[0] == 1.0
        d, i = fn(np.zeros((1, 3), np.float32), t[::-1].copy())
        assert i[0] == 0 and d[0] == 1.0
    d, i = CO.nearest(np.zeros((2, 3), np.float32), np.zeros((0, 3), np.float32))
    assert np.isinf(d).all() and (i == -1).all()


def _down_sample_plain(p, vs):
    lo = p.min(axis=0)
    org = [float(lo[a]) - 0.5 * vs for a in range(3)]
    cells = {}
    for row in p:
        k = tuple(int(np.floor((float(row[a]) - org[a]) / vs)) for a in range(3))
        cells.setdefault(k, []).append(row)
    pts, cnt = [], []
    for k in sorted(cells):
        s = [0.0, 0.0, 0.0]
        for row in cells[k]:
            for a in range(3):
                s[a] += float(row[a])
        pts.append([np.float32(s[a] / float(len(cells[k]))) for a in range(3)])
        cnt.append(len(cells[k]))
    return np.array(pts, np.float32).reshape(-1, 3), np.array(cnt, np.int32)


@pytest.mark.parametrize("offset", [0.0, 1000.0, -3.0])
def test_down_sample_oracle_equals_plain_implementation(offset):
    rng = np.random.default_rng(5)
    p = (rng.uniform(0, 0.3, (3000, 3)) + offset).astype(np.float32)
    p[100:140] = p[100]                                          # a crowded voxel: the order of the sum matters
    got_p, got_c = CO.down_sample(p, 0.02)
    exp_p, exp_c = _down_sample_plain(p, 0.02)
    assert np.array_equal(got_c, exp_c) and got_c.sum() == len(p)
    assert np.array_equal(got_p.view(np.uint32), exp_p.view(np.uint32))


def test_down_sample_oracle_rejects():
    with pytest.raises(ValueError):
        CO.down_sample(np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32), 0.02)
    with pytest.raises(ValueError):
        CO.down_sample(np.array([[0, 0, 0], [1e6, 0, 0]], np.float32), 0.02)
    p, c = CO.down_sample(np.zeros((0, 3), np.float32), 0.02)
    assert p.shape == (0, 3) and c.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------
# PLY reader
# ---------------------------------------------------------------------------------------------------------------
def test_ply_round_trips_mesh_export(tmp_path):
    import torch
    from cnrma_amd import cloud, mesh
    rng = np.random.default_rng(0)
    v = rng.normal(size=(37, 3)).astype(np.float32)
    m = mesh.Mesh(torch.from_numpy(v), torch.from_numpy(rng.integers(0, 37, (11, 3)).astype(np.int32)),
                  torch.from_numpy(rng.normal(size=(37, 3)).astype(np.float32)))
    path = str(tmp_path / "m.ply")
    m.cpu().export(path)
    got = cloud.read_ply_points(path)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), v.view(np.uint32))


def test_ply_ascii(tmp_path):
    from cnrma_amd import cloud
    path = tmp_path / "a.ply"
    path.write_text("ply\nformat ascii 1.0\ncomment hand written\nelement vertex 3\nproperty float x\nproperty float y\n"
                    "property uchar red\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                    "0 1 255 2\n-1.5 2.25 0 1e-3\n3 4 7 5\n3 0 1 2\n")
    assert np.array_equal(cloud.read_ply_points(str(path)), np.array([[0, 1, 2], [-1.5, 2.25, 1e-3], [3, 4, 5]], np.float32))


@pytest.mark.parametrize("end,fmt", [("<", "binary_little_endian"), (">", "binary_big_endian")])
def test_ply_binary_with_colours_and_faces(tmp_path, end, fmt):
    from cnrma_amd import cloud
    v = np.random.default_rng(1).normal(size=(5, 3)).astype(np.float32)
    path = tmp_path / "b.ply"
    head = (f"ply\nformat {fmt} 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    body = b"".join(struct.pack(end + "fffBBBB", *row, 1, 2, 3, 255) for row in v.tolist())
    path.write_bytes(head.encode("ascii") + body + struct.pack(end + "Biii", 3, 0, 1, 2))
    assert np.array_equal(cloud.read_ply_points(str(path)).view(np.uint32), v.view(np.uint32))


def test_ply_double_precision_is_rounded(tmp_path):
    from cnrma_amd import cloud
    v = np.random.default_rng(2).normal(size=(4, 3))
    path = tmp_path / "d.ply"
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\nend_header\n"
    path.write_bytes(head.encode("ascii") + v.astype("<f8").tobytes())
    assert np.array_equal(cloud.read_ply_points(str(path)), v.astype(np.float32))


def test_ply_rejects(tmp_path):
    from cnrma_amd import cloud
    a = tmp_path / "face_first.ply"
    a.write_text("ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nelement vertex 0\n"
                 "property float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError, match="face"):
        cloud.read_ply_points(str(a))
    b = tmp_path / "list_in_vertex.ply"
    b.write_text("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                 "property list uchar int neighbours\nend_header\n")
    with pytest.raises(ValueError, match="neighbours"):
        cloud.read_ply_points(str(b))
    c = tmp_path / "int_xyz.ply"
    c.write_text("ply\nformat ascii 1.0\nelement vertex 0\nproperty int x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError, match="x"):
        cloud.read_ply_points(str(c))


# ---------------------------------------------------------------------------------------------------------------
# the C-ABI table and the CLI
# ---------------------------------------------------------------------------------------------------------------
def test_cloud_signatures():
    from cnrma_amd import _lib
    arity = {"cnrma_cloud_downsample_workspace_bytes": 1, "cnrma_cloud_voxel_downsample_f32": 11,
             "cnrma_cloud_nn_workspace_bytes": 1, "cnrma_cloud_nn_build_f32": 7, "cnrma_cloud_nn_query_f32": 9,
             "cnrma_cloud_score_workspace_bytes": 1, "cnrma_cloud_score_f64": 8}
    for name, n in arity.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    import ctypes
    assert _lib.SIGNATURES["cnrma_cloud_voxel_downsample_f32"][1][3] is ctypes.c_double      # the voxel size is a double
    assert _lib.ABI_VERSION == 7


def test_cli_arguments_are_the_references():
    cli = _cli()
    args = cli.parse_args(["--data_path", "d", "--result_path", "r"])
    assert sorted(vars(args)) == ["axis_align", "data_path", "dataset", "result_path"]
    assert args.dataset == "arkit" and args.axis_align == 1
    a = cli.parse_args(["--dataset", "scannet", "--data_path", "/d", "--result_path", "/r", "--axis_align", "0"])
    pred, gt, m = cli.scene_files(a, "scene0001_00")
    assert pred == "/r/scene0001_00/scene0001_00.ply" and gt == "/d/scans/scene0001_00/scene0001_00_vh_clean_2.ply" and m is None
    a.dataset = "arkit"
    assert cli.scene_files(a, "42")[1] == "/d/3dod/Validation/42/42_3dod_mesh.ply"


def test_cli_axis_alignment(tmp_path):
    cli = _cli()
    p = tmp_path / "s.txt"
    p.write_text("colorHeight = 968\naxisAlignment = 0 1 0 2 -1 0 0 3 0 0 1 4 0 0 0 1 \nnumDepthFrames = 5\n")
    m = cli.read_axis_align_matrix(str(p))
    assert np.array_equal(m, np.array([[0, 1, 0, 2], [-1, 0, 0, 3], [0, 0, 1, 4], [0, 0, 0, 1]], np.float64))
    assert np.array_equal(cli.read_axis_align_matrix(str(tmp_path / "missing.txt")), np.eye(4))
