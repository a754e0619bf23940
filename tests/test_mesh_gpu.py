"""GPU tests of the device mesh extraction (cnrma_amd.mesh / csrc/mesh.hip) against the host oracle tests/mesh_oracle.py.

"Equals the oracle" means throughout: counts and faces equal as integers, vertices bit-equal in float32 (the formula is prescribed
and un-fused), normals within 1e-6 absolute (components <= 1; a handful of fp32 roundings is about 5e-7).  Several checks do not use
the case table at all (sign-change edge count, edge matching, signed volume), so that a wrong table cannot vouch for itself."""
import importlib.util
import os
import runpy
import sys

import numpy as np
import pytest
import torch

import mesh_oracle as MO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY_F, CANARY_I = -12345.5, -77


def _raw(vol, v_cap=None, f_cap=None, voxel_size=1.0, origin=(0.0, 0.0, 0.0), pad=8):
    """count + emit through the C ABI with chosen capacities; the output buffers are `pad` rows longer than the capacity and
    pre-filled with a canary.  -> counts [4], vertices, normals, faces (whole buffers, on the host)"""
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr, stream
    vol = vol.float().contiguous()
    dev = vol.device
    X, Y, Z = vol.shape
    nbytes = _lib.load().cnrma_mesh_workspace_bytes(X, Y, Z)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int32, device=dev)
    call("cnrma_mesh_count_f32", ptr(vol), X, Y, Z, ptr(ws), nbytes, ptr(counts), stream())
    c = counts.cpu().tolist()
    v_cap = c[0] if v_cap is None else v_cap
    f_cap = c[1] if f_cap is None else f_cap
    vert = torch.full((v_cap + pad, 3), CANARY_F, dtype=torch.float32, device=dev)
    norm = torch.full((v_cap + pad, 3), CANARY_F, dtype=torch.float32, device=dev)
    face = torch.full((f_cap + pad, 3), CANARY_I, dtype=torch.int32, device=dev)
    org = torch.tensor(origin, dtype=torch.float32, device=dev)
    call("cnrma_mesh_emit_f32", ptr(vol), X, Y, Z, float(voxel_size), ptr(org), ptr(ws), ptr(vert), ptr(norm), v_cap, ptr(face),
         f_cap, ptr(counts), stream())
    torch.cuda.synchronize()
    return c, vert.cpu().numpy(), norm.cpu().numpy(), face.cpu().numpy()


def _assert_equals_oracle(v, device, voxel_size=1.0, origin=None):
    """marching_cubes(v) on the device against the oracle; returns (device mesh as numpy arrays, oracle result)"""
    from cnrma_amd import mesh
    exp = MO.marching_cubes(v, voxel_size, origin)
    got = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(v)).to(device), voxel_size, origin).cpu()
    gv, gn, gf = got.vertices.numpy(), got.vertex_normals.numpy(), got.faces.numpy()
    assert gv.shape == exp["vertices"].shape and gf.shape == exp["faces"].shape and gn.shape == gv.shape
    assert gv.dtype == np.float32 and gf.dtype == np.int32
    assert np.array_equal(gf, exp["faces"])
    assert np.array_equal(gv.view(np.uint32), exp["vertices"].view(np.uint32))
    assert np.abs(gn - exp["normals"]).max(initial=0.0) <= 1e-6
    return (gv, gn, gf), exp


def _random_field(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def test_all_256_cases_in_one_launch(device):
    """the 256 shelled 4x4x4 blocks concatenated along x -> [1024,4,4]: equals the oracle, closed and oriented"""
    rng = np.random.default_rng(1)
    g = np.concatenate([MO.case_block(c, rng) for c in range(256)], axis=0)
    assert g.shape == (1024, 4, 4)
    (gv, _, gf), exp = _assert_equals_oracle(MO.tsdf_of_field(g), device)
    c, _, _, _ = _raw(torch.from_numpy(MO.tsdf_of_field(g)).to(device))
    assert tuple(c[:3]) == exp["counts"] and c[3] == 3
    assert len(gv) == MO.sign_change_edges(g)
    assert MO.is_closed_and_oriented(gf) and MO.signed_volume(gv, gf) > 0


@pytest.mark.parametrize("shape", [(2, 2, 2), (8, 7, 6), (3, 70, 5), (5, 3, 65), (4, 3, 130), (33, 17, 67)])
def test_edge_geometry_shelled(device, shape):
    """random fields in (-1, 1) inside a -1 shell; z runs of 65 / 130 cross a wave and a workgroup.  At (2,2,2) the shell would
    be the whole volume (no surface at all), so the single cell keeps its random corners: its surface ends on the cell's faces and
    cannot be closed, and only the comparison and the vertex count apply to it"""
    g = _random_field(shape, seed=sum(shape))
    if shape != (2, 2, 2):
        g = MO.shelled(g)
    (gv, _, gf), exp = _assert_equals_oracle(MO.tsdf_of_field(g), device)
    assert len(gv) > 0 and len(gf) > 0
    assert len(gv) == MO.sign_change_edges(g)                                 # table-free 1
    if shape != (2, 2, 2):
        assert MO.is_closed_and_oriented(gf)                                  # table-free 2
        assert MO.signed_volume(gv, gf) > 0                                   # table-free 3


@pytest.mark.parametrize("shape", [(2, 2, 2), (8, 7, 6), (3, 70, 5), (5, 3, 65), (4, 3, 130), (33, 17, 67)])
def test_open_surface(device, shape):
    """the same fields without the shell: equals the oracle, and every unmatched edge lies in a border face of the volume"""
    g = _random_field(shape, seed=sum(shape))
    (gv, _, gf), _ = _assert_equals_oracle(MO.tsdf_of_field(g), device)
    assert len(gv) == MO.sign_change_edges(g)
    _, unmatched = MO.edge_stats(gf)
    a, b = gv[unmatched[:, 0]], gv[unmatched[:, 1]]
    top = np.asarray(shape, dtype=np.float32) - 1
    on_face = ((a == 0) & (b == 0)) | ((a == top) & (b == top))
    assert on_face.any(axis=1).all()
    if min(shape) > 2:
        assert len(unmatched) > 0


def test_reference_field_transform(device):
    """exact 1.0 voxels (unobserved -> inside) next to negative ones, and values outside [-1, 1] (clamped): equals the oracle on
    the transformed field; no vertex on an edge between a v == 1 voxel and a v < 0 voxel (both are inside)"""
    rng = np.random.default_rng(7)
    v = rng.uniform(-1.6, 1.6, (9, 10, 11)).astype(np.float32)
    v[rng.uniform(size=v.shape) < 0.3] = 1.0
    v[2:5, 3:6, 4:8] = 1.0
    v[2:5, 6, 4:8] = -0.4
    assert (np.abs(v) > 1).any() and (v == 1).sum() > 100
    (gv, _, _), exp = _assert_equals_oracle(v, device)
    g = MO.field(v)
    assert len(gv) == MO.sign_change_edges(g) and len(gv) > 0
    assert g.max() == 1 and g.min() == -1
    frac = np.abs(gv - np.rint(gv))
    axis = frac.argmax(axis=1)
    assert (frac.max(axis=1) > 0).all()                                        # no vertex sits on a voxel here
    lo = np.rint(gv).astype(np.int64)
    lo[np.arange(len(gv)), axis] = np.floor(gv[np.arange(len(gv)), axis]).astype(np.int64)
    hi = lo.copy()
    hi[np.arange(len(gv)), axis] += 1
    v0, v1 = v[lo[:, 0], lo[:, 1], lo[:, 2]], v[hi[:, 0], hi[:, 1], hi[:, 2]]
    assert not (((v0 == 1) & (v1 < 0)) | ((v1 == 1) & (v0 < 0))).any()
    assert (((v == 1)[:-1] & (v < 0)[1:]).sum()) > 0                            # such edges do exist in the volume


def _empty_volumes():
    rng = np.random.default_rng(3)
    pos = rng.uniform(0.05, 0.95, (6, 5, 7)).astype(np.float32)
    zeros = rng.uniform(size=pos.shape) < 0.3
    return {"all v > 0": pos, "all v < 0": -pos, "v <= 0 with zeros": np.where(zeros, 0, -pos).astype(np.float32),
            "v >= 0 with zeros": np.where(zeros, 0, pos).astype(np.float32), "constant": np.full(pos.shape, -0.25, np.float32)}


@pytest.mark.parametrize("name", list(_empty_volumes()))
def test_empty_meshes(device, name):
    """The reference (tsdf.py:106-107) returns an empty mesh when min(g) >= 0 or max(g) <= 0, g = the transformed field.  Both
    zero-mixed volumes are therefore empty: v <= 0 gives g >= 0 (min >= 0) and v >= 0 gives g <= 0 (max <= 0) -- although g == 0
    counts as outside for the cases, so that the first of them does have sign-change edges.  Rule: a mesh needs one voxel with
    g < 0 AND one with g > 0.  The output buffers stay untouched."""
    from cnrma_amd import mesh
    v = _empty_volumes()[name]
    assert MO.marching_cubes(v)["counts"] == (0, 0, 0)
    c, vert, norm, face = _raw(torch.from_numpy(v).to(device), v_cap=16, f_cap=16)
    assert c[:3] == [0, 0, 0]
    g = MO.field(v)
    assert c[3] == (1 if (g < 0).any() else 0) | (2 if (g > 0).any() else 0)
    assert (vert == CANARY_F).all() and (norm == CANARY_F).all() and (face == CANARY_I).all()
    m = mesh.marching_cubes(torch.from_numpy(v).to(device))
    assert tuple(m.vertices.shape) == (0, 3) and tuple(m.faces.shape) == (0, 3) and tuple(m.vertex_normals.shape) == (0, 3)
    if name == "v <= 0 with zeros":
        assert MO.sign_change_edges(g) > 0


def test_capacity(device):
    """capacities one short of the need, and 0: nothing is written at or beyond them, what lies below equals the full result,
    and counts still report the true need; marching_cubes sizes exactly"""
    from cnrma_amd import mesh
    v = MO.tsdf_of_field(MO.shelled(_random_field((8, 7, 6), seed=21)))
    dv = torch.from_numpy(v).to(device)
    c, vert, norm, face = _raw(dv)
    nv, nf = c[0], c[1]
    exp = MO.marching_cubes(v)
    assert (nv, nf) == exp["counts"][:2] and nv > 8 and nf > 8
    assert np.array_equal(face[:nf], exp["faces"]) and np.array_equal(vert[:nv], exp["vertices"])
    assert (vert[nv:] == CANARY_F).all() and (norm[nv:] == CANARY_F).all() and (face[nf:] == CANARY_I).all()
    for v_cap, f_cap in ((nv - 1, nf - 1), (0, 0), (nv, 0), (0, nf)):
        c2, vert2, norm2, face2 = _raw(dv, v_cap=v_cap, f_cap=f_cap)
        assert c2 == c
        assert np.array_equal(vert2[:v_cap], vert[:v_cap]) and np.array_equal(norm2[:v_cap], norm[:v_cap])
        assert np.array_equal(face2[:f_cap], face[:f_cap])
        assert (vert2[v_cap:] == CANARY_F).all() and (norm2[v_cap:] == CANARY_F).all() and (face2[f_cap:] == CANARY_I).all()
    m = mesh.marching_cubes(dv)
    assert tuple(m.vertices.shape) == (nv, 3) and tuple(m.faces.shape) == (nf, 3)


def _sinusoids(shape, fx=0.21):
    i, j, k = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in shape), indexing="ij", sparse=True)
    return (0.5 * np.sin(i * fx + 0.3) + 0.3 * np.sin(j * 0.17 + 1.1) + 0.19 * np.sin(k * 0.29 + 2.0)).astype(np.float32)


def test_multi_block_scan_and_compaction(device):
    """A smooth field (three sinusoids) at 104^3 instead of 96^3: the scan here runs over the totals of RUNS of 1024 voxels (one
    wave each), not of 256-voxel blocks, and its one 1024-thread block gives every thread more than one total only above 1024 runs
    = 1048576 voxels (about 101.6^3; 96^3 is 864 runs and would stay on the one-total path).  104^3 = 1099 runs is the smallest
    cube on a multiple of 8 that crosses it; its tens of thousands of list entries are far more than one block of the compaction or
    of the emit.  Equals the oracle; two runs on different streams are bit-identical"""
    from cnrma_amd import mesh
    g = _sinusoids((104, 104, 104))
    v = MO.tsdf_of_field(g)
    (gv, gn, gf), exp = _assert_equals_oracle(v, device)
    assert g.size > 1024 * 1024 and exp["counts"][2] > 20000 and len(gv) == MO.sign_change_edges(g)
    dv = torch.from_numpy(v).to(device)
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=device)
        s.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(s):
            m = mesh.marching_cubes(dv)
        s.synchronize()
        runs.append(m.cpu())
    for m in runs:
        assert np.array_equal(m.vertices.numpy().view(np.uint32), gv.view(np.uint32))
        assert np.array_equal(m.vertex_normals.numpy().view(np.uint32), gn.view(np.uint32))
        assert np.array_equal(m.faces.numpy(), gf)


def test_scan_stretch_longer_than_one_load_batch(device):
    """the scan block loads each thread's stretch of run totals eight at a time; above 8192 runs (8.4 M voxels, the size of the
    shipped 192^3 / 256x256x96 volumes) a stretch needs a second batch.  [2064,64,64] = 8256 runs is just past it, with a field that
    varies slowly along x to keep the oracle to a few seconds"""
    g = _sinusoids((2064, 64, 64), fx=0.02)
    assert g.size == 8256 * 1024
    (gv, _, gf), exp = _assert_equals_oracle(MO.tsdf_of_field(g), device)
    assert exp["counts"][2] > 100000 and len(gv) == MO.sign_change_edges(g)


def test_sphere(device):
    """24^3, centre 11.3, v = clamp((r - 8) / 3, -1, 1) (MO.sphere_tsdf: the saturated far side as 2, not as the "unobserved" marker
    1).  Tolerances are the oracle's own figures against the ANALYTIC sphere, measured on the CPU (tests/test_mesh_cpu.py): largest
    radial error 0.0151 voxel; volume 2124.6 of 4/3 pi 8^3 = 2144.7 (inscribed triangles under-estimate a convex body); smallest
    normal . radial 0.9999945"""
    (gv, gn, gf), _ = _assert_equals_oracle(MO.sphere_tsdf(), device)
    v = gv.astype(np.float64)
    r = np.linalg.norm(v - 11.3, axis=1)
    assert np.abs(r - 8).max() < 0.02
    vol, exact = MO.signed_volume(v, gf), 4.0 / 3.0 * np.pi * 8.0 ** 3
    assert 0.985 * exact <= vol < exact
    assert MO.is_closed_and_oriented(gf) and MO.edge_stats(gf)[0] == 0 and MO.euler_characteristic(len(v), gf) == 2
    dots = ((v - 11.3) / r[:, None] * gn).sum(axis=1)
    assert (dots > 0).all() and dots.min() > MO.SPHERE_MIN_DOT


def _base(tmp_path, **kw):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.models.multiview_base import MultiViewBase
    return MultiViewBase(pixel_mean=[0, 0, 0], pixel_std=[1, 1, 1], voxel_size=0.04, n_scales=2, voxel_dim_train=[16, 16, 16],
                         voxel_dim_test=[16, 16, 16], origin=[0, 0, 0], backbone2d_stride=4, backbone2d=None, feature_2d=None,
                         backbone_3d=None, tsdf_head=None, save_path=str(tmp_path), **kw)


def test_wiring(device, tmp_path):
    """TSDF.get_mesh_device applies voxel_size and origin; save_reconstruction with mesh_extractor="device" writes {scene}.ply =
    marching_cubes' arrays; with the default and no scikit-image no .ply appears; the CLI rebuilds the same file from the .npz"""
    from cnrma_amd import mesh
    from projects.mvsdetection.datasets.tsdf import TSDF
    i, j, k = np.indices((16, 16, 16)).astype(np.float32)
    v = np.clip((np.sqrt((i - 7.4) ** 2 + (j - 8.1) ** 2 + (k - 6.7) ** 2) - 5) / 3, -0.99, 0.99).astype(np.float32)
    vol = torch.from_numpy(v).to(device)
    offset = torch.tensor([0.25, -0.5, 0.125], device=device)
    exp = MO.marching_cubes(v, 0.04, offset.cpu().numpy())
    m = TSDF(0.04, offset.view(1, 3), vol).get_mesh_device().cpu()
    assert np.array_equal(m.vertices.numpy(), exp["vertices"]) and np.array_equal(m.faces.numpy(), exp["faces"])
    unit = mesh.marching_cubes(vol).cpu()
    assert len(exp["vertices"]) > 100 and not np.array_equal(unit.vertices.numpy(), m.vertices.numpy())

    outputs, inputs = {"scene_tsdf_004": vol.view(1, 1, 16, 16, 16)}, {"offset": [offset], "scene": ["sc0"]}
    _base(tmp_path / "dev", mesh_extractor="device").save_reconstruction(outputs, inputs)
    ply = tmp_path / "dev" / "sc0" / "sc0.ply"
    pv, pn, pf = MO.read_ply(ply)
    assert np.array_equal(pv, m.vertices.numpy()) and np.array_equal(pn, m.vertex_normals.numpy())
    assert np.array_equal(pf, m.faces.numpy())
    assert sorted(os.listdir(tmp_path / "dev" / "sc0")) == ["sc0.npz", "sc0.ply"]

    _base(tmp_path / "ref").save_reconstruction(outputs, inputs)
    if importlib.util.find_spec("skimage") is None:
        assert os.listdir(tmp_path / "ref" / "sc0") == ["sc0.npz"]

    first = open(ply, "rb").read()
    os.remove(ply)
    argv = sys.argv
    sys.argv = ["extract_mesh.py", "--result_path", str(tmp_path / "dev")]
    try:
        runpy.run_path(os.path.join(ROOT, "post_process", "extract_mesh.py"), run_name="__main__")
    finally:
        sys.argv = argv
    assert open(ply, "rb").read() == first
