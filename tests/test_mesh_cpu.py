"""Mesh extraction, the part that needs no GPU: the generated case table (cnrma_amd.mesh_table -> csrc/mesh_table.inc), its
validity checked geometrically through the host oracle (tests/mesh_oracle.py) without trusting the table's own book-keeping,
the PLY writer, and the plugin's mesh_extractor switch."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_reproduces_the_committed_table():
    """`python -m cnrma_amd.mesh_table` prints csrc/mesh_table.inc byte for byte; at most 5 triangles per case, 820 over all"""
    from cnrma_amd import mesh_table
    out = subprocess.run([sys.executable, "-m", "cnrma_amd.mesh_table"], cwd=ROOT, check=True, capture_output=True).stdout
    committed = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "mesh_table.inc"), "rb").read()
    assert out == committed
    n = [len(t) for t in mesh_table.TABLE]
    assert len(n) == 256 and max(n) == 5 == mesh_table.MAX_TRIANGLES and sum(n) == 820
    assert n[0] == 0 and n[255] == 0 and all(k > 0 for k in n[1:255])


def test_makefile_builds_the_table_into_both_libraries():
    mk = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    rule = [ln for ln in mk.splitlines() if ln.startswith("mesh.o:")]
    assert len(rule) == 1 and "mesh_table.inc" in rule[0] and "mesh.hip" in rule[0]
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0]
    exp = [ln for ln in mk.splitlines() if ln.startswith("EXP_OBJS")][0]
    assert "mesh.hip" in srcs.split() and "mesh.o" in exp.split()


def test_every_case_is_closed_oriented_and_encloses_its_inside_corners():
    """each of the 256 cases as the central cell of a 4x4x4 volume with a -1 shell and inside corners drawn from (0.1, 1): every
    directed edge occurs once and its opposite once (closed, consistently oriented, edge-manifold), and the signed volume is
    positive (the triangles face away from the inside corners)"""
    rng = np.random.default_rng(1)
    for case in range(256):
        g = MO.case_block(case, rng)
        v = MO.tsdf_of_field(g)
        assert (MO.field(v) == g).all()
        m = MO.marching_cubes(v)
        if case == 0:
            assert m["counts"] == (0, 0, 0)
            continue
        assert m["counts"][0] == MO.sign_change_edges(g)
        dup, unmatched = MO.edge_stats(m["faces"])
        assert dup == 0 and len(unmatched) == 0, case
        assert MO.signed_volume(m["vertices"], m["faces"]) > 0, case
        assert m["faces"].min() == 0 and m["faces"].max() == m["counts"][0] - 1


def test_oracle_on_random_shelled_volumes_and_the_sphere():
    """the oracle itself: closed, oriented, one vertex per sign-change edge, positive volume; and the sphere figures that the GPU
    test's tolerances come from (radial error 0.0151 voxel, volume 2124.6 of 2144.7, Euler characteristic 2)"""
    rng = np.random.default_rng(2)
    for _ in range(5):
        g = MO.shelled(rng.uniform(-1, 1, (8, 7, 6)).astype(np.float32))
        m = MO.marching_cubes(MO.tsdf_of_field(g))
        assert MO.is_closed_and_oriented(m["faces"]) and m["counts"][0] == MO.sign_change_edges(g)
        assert MO.signed_volume(m["vertices"], m["faces"]) > 0
    m = MO.marching_cubes(MO.sphere_tsdf())
    v = m["vertices"].astype(np.float64)
    r = np.linalg.norm(v - 11.3, axis=1)
    assert abs(np.abs(r - 8).max() - 0.0151) < 1e-4
    assert abs(MO.signed_volume(v, m["faces"]) - 2124.6) < 0.05
    assert MO.is_closed_and_oriented(m["faces"]) and MO.euler_characteristic(len(v), m["faces"]) == 2
    dots = ((v - 11.3) / r[:, None] * m["normals"]).sum(1)
    assert dots.min() > MO.SPHERE_MIN_DOT                     # the measured minimum is 0.9999945


def test_the_reference_empty_rule_in_the_oracle():
    """reference tsdf.py:106-107 returns an empty mesh when min(g) >= 0 or max(g) <= 0: exact zeros do not make a surface on
    their own, although g == 0 counts as outside when cells are classified"""
    z = np.zeros((4, 4, 4), np.float32)
    z[1:3, 1:3, 1:3] = 0.5                                    # v >= 0 with zeros: g <= 0
    assert MO.marching_cubes(z)["counts"] == (0, 0, 0) and MO.marching_cubes(-z)["counts"] == (0, 0, 0)
    z[0, 0, 0] = -0.5
    assert MO.marching_cubes(z)["counts"][0] > 0


def _mesh(nv, nf, seed=0):
    from cnrma_amd import mesh
    g = torch.Generator().manual_seed(seed)
    return mesh.Mesh(torch.randn(nv, 3, generator=g), torch.randint(0, max(nv, 1), (nf, 3), generator=g, dtype=torch.int32),
                     torch.randn(nv, 3, generator=g))


@pytest.mark.parametrize("nv,nf", [(7, 11), (0, 0)])
def test_ply_round_trip(tmp_path, nv, nf):
    m = _mesh(nv, nf)
    path = tmp_path / "m.ply"
    m.export(str(path))
    v, n, f = MO.read_ply(path)
    assert v.shape == (nv, 3) and f.shape == (nf, 3)
    assert np.array_equal(v, m.vertices.numpy()) and np.array_equal(n, m.vertex_normals.numpy())
    assert np.array_equal(f, m.faces.numpy()) and f.dtype == np.int32
    assert os.listdir(tmp_path) == ["m.ply"]                  # the temporary name is gone
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    assert f"element vertex {nv}\n" in head and f"element face {nf}\n" in head


def test_mesh_extractor_keyword():
    """MultiViewBase takes mesh_extractor=None | "device", RayMarching and Atlas pass it through, anything else is refused;
    without a GPU the device path raises the library's error instead of falling back"""
    import projects.mvsdetection  # noqa: F401
    from cnrma_amd import _lib
    from projects.mvsdetection.datasets.tsdf import TSDF
    from projects.mvsdetection.models.atlas import Atlas
    from projects.mvsdetection.models.multiview_base import MultiViewBase
    from projects.mvsdetection.models.ray_marching import RayMarching
    for cls in (MultiViewBase, RayMarching, Atlas):
        assert inspect.signature(cls.__init__).parameters["mesh_extractor"].default is None
    kw = dict(pixel_mean=[0, 0, 0], pixel_std=[1, 1, 1], voxel_size=0.04, n_scales=2, voxel_dim_train=[8, 8, 8],
              voxel_dim_test=[8, 8, 8], origin=[0, 0, 0], backbone2d_stride=4, backbone2d=None, feature_2d=None, backbone_3d=None,
              tsdf_head=None, save_path=None)
    assert MultiViewBase(**kw).mesh_extractor is None and MultiViewBase(mesh_extractor="device", **kw).mesh_extractor == "device"
    with pytest.raises(ValueError):
        MultiViewBase(mesh_extractor="skimage", **kw)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.CnrmaError):
            TSDF(0.04, torch.zeros(1, 3), torch.zeros(4, 4, 4)).get_mesh_device()


def test_workspace_size_is_host_arithmetic():
    lib = __import__("cnrma_amd._lib", fromlist=["load"]).load()
    size = lib.cnrma_mesh_workspace_bytes
    assert size(0, 4, 4) == 0 and size(4, -1, 4) == 0 and size(1024, 1024, 1024) == 0
    n = 192 ** 3
    assert 9 * n <= size(192, 192, 192) <= 9.25 * n and size(192, 192, 192) % 8 == 0
    assert size(2, 2, 2) >= 64 + 2 * 16 + 64 + 8 * 8
