"""CPU suite (-m "not gpu"): the oracle against the committed golden vectors (generated from the reference's own
Python by tests/golden/make_golden.py), the host logic, and the C-ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import EDGE_SCENES, QUIRK_SCENES, QUIRK_SINGLE_VIEW, SCENES, bits_equal, count_mismatch, edge_facts, load_golden, t
from oracle import rma_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", SCENES)
def test_oracle_dense_matches_golden(name):
    g = load_golden(name)
    vol, cnt = O.backproject_accum(g["dims"], g["voxel_size"], g["origin"], t(g["projection"]), t(g["features"]),
                                   g["stride"])
    assert count_mismatch(vol, g["dense_volume"]) == 0
    assert (cnt.numpy() == g["dense_count"]).all()
    _, valid, px, py = O.backproject_view(g["dims"], g["voxel_size"], g["origin"],
                                          O.scale_projection(t(g["projection"][0]), g["stride"]), t(g["features"][0]))
    assert (px.numpy() == g["view0_px"]).all() and (py.numpy() == g["view0_py"]).all()
    assert (valid.numpy() == g["view0_valid"]).all()


@pytest.mark.parametrize("name", SCENES)
def test_oracle_ray_params_match_golden(name):
    g = load_golden(name)
    H, W = g["features"].shape[-2:]
    for v in range(g["features"].shape[0]):
        o, d = O.ray_params(O.scale_projection(t(g["projection"][v]), g["stride"]), H, W)
        assert count_mismatch(o, g["ray_o"][v]) == 0
        assert count_mismatch(d, g["ray_d"][v]) == 0


@pytest.mark.parametrize("name", SCENES)
def test_oracle_neus_rows_and_points_match_golden(name):
    g = load_golden(name)
    tsdf = t(g["tsdf"])
    rows, counts = [], []
    for v in range(g["features"].shape[0]):
        r = O.rma_neus_view(O.scale_projection(t(g["projection"][v]), g["stride"]), t(g["features"][v]), tsdf,
                            g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"])
        counts.append(0 if r is None else r.shape[0])
        if r is not None:
            rows.append(r)
    assert counts == list(g["neus_counts"])
    assert count_mismatch(torch.cat(rows), g["neus_rows"]) == 0
    pts = O.aggregate_rma(t(g["projection"]), t(g["features"]), tsdf, g["dims"], g["voxel_size"], g["origin"],
                          g["stride"], 300, g["thr"])
    assert count_mismatch(pts, g["points"]) == 0


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_oracle_depth_rows_match_golden(name, k):
    g = load_golden(name)
    r = O.rma_depth_view(O.scale_projection(t(g["projection"][0]), g["stride"]), t(g["features"][0]), t(g["tsdf"]),
                         g["dims"], g["voxel_size"], g["origin"], g["n_steps"], k)
    exp = g[f"depth_rows_k{k}"]
    if exp.shape[0] == 0:
        assert r is None
    else:
        assert count_mismatch(r, exp) == 0


@pytest.mark.parametrize("name", SCENES)
def test_oracle_select_and_voxelize_match_golden(name):
    g = load_golden(name)
    M = g["points"].shape[0]
    mask = np.unpackbits(g["sel_mask"])[:M].astype(bool)
    # the mask is what numpy's global RNG gives under the recorded seed (sample_points semantics)
    np.random.seed(7)
    assert (O.sample_mask_numpy(M, int(g["sel_max_points"])) == mask).all()
    c, f = O.select_rows(t(g["points"]), g["sel_offset"], mask)
    assert count_mismatch(c, g["sel_coords"]) == 0 and count_mismatch(f, g["sel_feats"]) == 0
    Cq, Fq, src = O.voxelize(c, f, 0.01)
    assert (Cq.numpy() == g["vox_coords"]).all() and (src.numpy() == g["vox_src"]).all()
    # first-wins: every source index is the smallest index of its voxel
    q = torch.floor(c / 0.01).to(torch.int32).numpy()
    seen = {}
    for i, row in enumerate(map(tuple, q)):
        seen.setdefault(row, i)
    assert sorted(seen.values()) == list(src.numpy())


def test_all_views_empty_raises_like_reference():
    g = load_golden("edge_empty_view")
    with pytest.raises(TypeError):
        O.aggregate_rma(t(g["projection"][:1]), t(g["features"][:1]), t(g["tsdf"]), g["dims"], g["voxel_size"],
                        g["origin"], g["stride"])


QUIRK_MODES = [("neus", None), ("depth", 0), ("depth", 1), ("depth", 2)]


@pytest.mark.parametrize("name", QUIRK_SCENES)
@pytest.mark.parametrize("mode,k", QUIRK_MODES)
def test_oracle_drops_single_sample_views_like_reference(name, mode, k):
    """a view that keeps exactly one sample is skipped by the reference (ray_marching.py:781-782 / :930-931 raise inside
    the bare except of :277-287): per-view rows, skipped views and the scene aggregate of the reference's own loop"""
    g = load_golden(name)
    tag = "neus" if mode == "neus" else f"depth_k{k}"
    tsdf = t(g["tsdf"])
    rows, raw_single = [], []
    for v in range(g["features"].shape[0]):
        args = (O.scale_projection(t(g["projection"][v]), g["stride"]), t(g["features"][v]), tsdf, g["dims"],
                g["voxel_size"], g["origin"], g["n_steps"])
        if mode == "neus":
            r = O.rma_neus_view(*args, g["thr"])
            raw = O.rma_neus_view(*args, g["thr"], reference_quirks=False)
        else:
            r = O.rma_depth_view(*args, k)
            raw = O.rma_depth_view(*args, k, reference_quirks=False)
        if g[f"{tag}_skipped"][v]:
            assert r is None and raw is not None and raw.shape[0] == 1, v
            raw_single.append(raw)
        else:
            assert (0 if r is None else r.shape[0]) == g[f"{tag}_counts"][v], v
            if r is not None:
                assert count_mismatch(r, raw) == 0
                rows.append(r)
    exp_rows = g[f"{tag}_rows"]
    assert count_mismatch(torch.cat(rows) if rows else torch.zeros(exp_rows.shape), exp_rows) == 0
    exp_single = g[f"{tag}_single_rows"]
    assert len(raw_single) == exp_single.shape[0] == int(g[f"{tag}_skipped"].sum())
    if raw_single:
        assert count_mismatch(torch.cat(raw_single), exp_single) == 0
    agg = (t(g["projection"]), t(g["features"]), tsdf, g["dims"], g["voxel_size"], g["origin"], g["stride"], g["n_steps"],
           g["thr"], mode, k or 0)
    if g[f"{tag}_raises"]:
        with pytest.raises(TypeError):
            O.aggregate_rma(*agg)
    else:
        pts = O.aggregate_rma(*agg)
        assert count_mismatch(pts, g[f"{tag}_points"]) == 0
    # without the quirk the one-sample views come back: exactly one row more per skipped view
    if raw_single:
        full = O.aggregate_rma(*agg, reference_quirks=False)
        assert full.shape[0] == g[f"{tag}_points"].shape[0] + len(raw_single)


def test_quirk_fixtures_hold_the_cases_they_are_for():
    """the fixtures exercise what they are named for: a one-sample view among views that keep many, at view 0 and at
    view 1 (NeuS), and at view 0 in depth mode k = 0; for k >= 1 a hit ray emits >= 2 rows, so nothing is dropped"""
    a, b, d = (load_golden(n) for n in QUIRK_SCENES)
    assert list(a["neus_skipped"]) == [True, False, False] and min(a["neus_counts"][1:]) >= 100
    assert list(b["neus_skipped"]) == [False, True, False] and min(b["neus_counts"][[0, 2]]) >= 100
    assert list(d["depth_k0_skipped"]) == [True, False, False] and min(d["depth_k0_counts"][1:]) >= 50
    for g in (a, b, d):
        assert not g["depth_k1_skipped"].any() and not g["depth_k2_skipped"].any()


@pytest.mark.parametrize("name", EDGE_SCENES)
def test_edge_fixtures_hold_the_edges_they_are_for(name):
    """the edge fixtures keep testing what they claim (the facts make_golden.py asserts, re-derived with the oracle): rays
    with exactly-zero direction components, rays that start outside the grid, rays whose last kept NeuS sample is their last
    in-grid sample before they leave through free space, view-0 depth hits at the step before entry, voxels behind or on the
    plane of a camera, samples on the rounding tie x/vs = -0.5; no NeuS weight within 1e-6 of thr and no one-sample view"""
    f = edge_facts(load_golden(name))
    assert f["zero_dir"] > 0 and f["start_outside"] > 0 and f["exit_free"] > 0 and f["depth_before_entry"] > 0, f
    assert f["depth_le0"] > 0, f
    assert f["thr_margin"] > 1e-6 and f["single_views"] == 0, f
    if name == "edge_outside_axis":
        assert f["depth_eq0"] > 0, f                       # view 1 stands on the lattice plane of column 23
    else:
        assert f["tie"] > 0, f                             # view 0's grazing rays run in the plane x = ox - 0.5 vs


def test_single_view_of_one_sample_raises_like_reference():
    g = load_golden(QUIRK_SINGLE_VIEW)
    assert bool(g["neus_raises"]) and g["features"].shape[0] == 1
    args = (t(g["projection"]), t(g["features"]), t(g["tsdf"]), g["dims"], g["voxel_size"], g["origin"], g["stride"],
            g["n_steps"], g["thr"])
    with pytest.raises(TypeError):
        O.aggregate_rma(*args)
    assert O.aggregate_rma(*args, reference_quirks=False).shape[0] == 1


def _voxel_subset_cases():
    for name in SCENES + QUIRK_SCENES:
        g = load_golden(name)
        yield name, g["dims"], g["voxel_size"], g["origin"], t(g["projection"]), t(g["features"]), g["stride"]


@pytest.mark.parametrize("case", ["golden", "ragged"])
def test_backproject_voxels_equal_full_grid_bit_for_bit(case):
    """backproject_voxels / backproject_accum_voxels (the oracle of the north-star-size dense test, which samples voxels)
    == backproject_view / backproject_accum at every voxel, bit for bit: on every fixture, and on a grid whose bricks of
    16 x 16 x 32 are ragged (72 x 100 x 80); the gather-callable form gives the same values"""
    from cnrma_amd import synth
    if case == "golden":
        cases = list(_voxel_subset_cases())
    else:
        sc = synth.make_scene((6, 32, 60, 80, (72, 100, 80), 4), seed=4)
        cases = [("ragged", sc["dims"], sc["voxel_size"], sc["origin"], sc["projection"][:, 0], sc["features"][:, 0],
                  sc["stride"])]
    for name, dims, vs, origin, proj, feat, stride in cases:
        G = dims[0] * dims[1] * dims[2]
        gidx = torch.arange(G)
        vol, cnt = O.backproject_accum(dims, vs, origin, proj, feat, stride)
        vol2, cnt2 = O.backproject_accum_voxels(dims, vs, origin, proj, feat, stride, gidx)
        assert torch.equal(cnt.view(-1), cnt2), name
        assert count_mismatch(vol.view(vol.shape[0], -1), vol2) == 0, name
        assert int(cnt.max()) > 0
        ps = O.scale_projection(proj[0], stride)
        v0, ok0, px0, py0 = O.backproject_view(dims, vs, origin, ps, feat[0])
        perm = torch.randperm(G, generator=torch.Generator().manual_seed(1))[: G // 3]
        v1, ok1, px1, py1 = O.backproject_voxels(dims, vs, origin, ps, feat[0], perm)
        assert torch.equal(ok1, ok0[perm]) and torch.equal(px1, px0[perm]) and torch.equal(py1, py0[perm])
        assert count_mismatch(v1, v0[:, perm]) == 0
        H, W = feat.shape[-2:]
        gathers = [(lambda f: (lambda py, px: f[:, py, px]))(feat[v]) for v in range(feat.shape[0])]
        vol3, cnt3 = O.backproject_accum_voxels(dims, vs, origin, proj, gathers, stride, perm, hw=(H, W))
        assert torch.equal(cnt3, cnt.view(-1)[perm]) and count_mismatch(vol3, vol.view(vol.shape[0], -1)[:, perm]) == 0


def test_host_projection_inverse_matches_golden():
    from cnrma_amd import rma
    for name in SCENES:
        g = load_golden(name)
        pinv = rma.projection_inverse(t(g["projection"]), g["stride"])
        # same call as the oracle's, so identical on any one host; vs the golden (generated on the build container's
        # CPU) LAPACK may differ in the last bits on another CPU model
        for v in range(pinv.shape[0]):
            assert torch.equal(pinv[v], O.projection_inverse(O.scale_projection(t(g["projection"][v]), g["stride"])))
        np.testing.assert_allclose(pinv.numpy(), g["proj_inv"], rtol=1e-4, atol=1e-5)


def test_synth_scene_is_deterministic():
    from cnrma_amd import synth
    a = synth.make_scene("tiny", seed=3, boxes=2)
    b = synth.make_scene("tiny", seed=3, boxes=2)
    for k in ("features", "projection", "tsdf"):
        assert torch.equal(a[k], b[k])
    g = load_golden("tiny")
    c = synth.make_scene("tiny", seed=0)
    assert count_mismatch(c["features"][:, 0], g["features"]) == 0
    assert count_mismatch(c["projection"][:, 0], g["projection"]) == 0
    assert count_mismatch(c["tsdf"][0, 0], g["tsdf"]) == 0


# ---------------------------------------------------------------------------------------------------------------
# C-ABI surface: the library loads, exports every symbol of include/cnrma.h, and the ctypes binding agrees in arity and types
# ---------------------------------------------------------------------------------------------------------------
def _header_functions(experiments=False):
    """prototypes of include/cnrma.h: the product surface, or (experiments=True) only those under #ifdef CNRMA_EXPERIMENTS"""
    src = open(os.path.join(ROOT, "include", "cnrma.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    exp = "\n".join(re.findall(r"#ifdef CNRMA_EXPERIMENTS\n(.*?)#endif", src, flags=re.S))
    src = exp if experiments else re.sub(r"#ifdef CNRMA_EXPERIMENTS\n.*?#endif", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int|size_t)\s+(cnrma_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        out[m.group(2)] = ([] if args in ("", "void") else [_kind(a) for a in args.split(",")], _kind(m.group(1) + " f"))
    return out


# name -> (parameters, return value), each a (class, bytes) pair taken from the C text; class: "pointer", "integer" or "floating"
_C_SCALARS = (("integer", 8, r"(u?int64_t|size_t)"), ("integer", 4, r"(int|u?int32_t)"), ("floating", 4, "float"), ("floating", 8, "double"))


def _kind(param):
    """(class, bytes) of one parameter's C text, name included: what a binding of it has to be, whatever it is called"""
    if "*" in param:
        return "pointer", ctypes.sizeof(ctypes.c_void_p)
    for cls, width, pat in _C_SCALARS:
        if re.fullmatch(rf"\s*(const\s+)?{pat}(\s+const)?\s+\w+\s*", param):
            return cls, width
    raise AssertionError(f"include/cnrma.h: a parameter this test cannot class: {param!r}")


def _bound_kind(ctype):
    """(class, bytes) of a ctypes type as ctypes itself treats it"""
    if ctype is ctypes.c_void_p:
        return "pointer", ctypes.sizeof(ctype)
    code = ctype._type_                      # struct-style type code of a simple ctypes type
    assert code in "fdbBhHiIlLqQ", ctype
    return ("floating" if code in "fd" else "integer"), ctypes.sizeof(ctype)


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}


def test_library_exports_every_declared_symbol():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.EXP_LIB_PATH):   # fresh checkout: hipcc cross-compiles without a GPU
        import subprocess
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH), "-j8"], check=True)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decl = _header_functions()
    assert len(decl) >= 30
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in include/cnrma.h but not exported"
    assert lib.cnrma_abi_version() == _lib.ABI_VERSION
    # the product library exports exactly the product surface: no cnrma_debug_* hook, nothing undeclared
    product = _exported(_lib.LIB_PATH)
    assert product == set(decl), product ^ set(decl)
    assert not [n for n in product if n.startswith("cnrma_debug")]
    # the experiments library = the same surface + the prototypes under #ifdef CNRMA_EXPERIMENTS
    extra = _header_functions(experiments=True)
    assert extra and all(n.startswith("cnrma_debug_") for n in extra)
    assert _exported(_lib.EXP_LIB_PATH) == set(decl) | set(extra)
    assert ctypes.CDLL(_lib.EXP_LIB_PATH).cnrma_abi_version() == _lib.ABI_VERSION


def test_ctypes_table_matches_header():
    """two readers of include/cnrma.h written separately -- the product's (_lib._read_header) and this file's regex -- agree on
    the names, the arity, and for every parameter and return value on its class (pointer / integer / floating) and width: a
    pointer bound as an int would be cut to 32 bits, a float bound as a double would arrive as garbage"""
    from cnrma_amd import _lib
    for decl, table in ((_header_functions(), _lib.SIGNATURES), (_header_functions(experiments=True), _lib.EXPERIMENT_SIGNATURES)):
        assert set(decl) == set(table), set(decl) ^ set(table)
        for name, (params, returns) in decl.items():
            restype, argtypes = table[name]
            assert len(argtypes) == len(params), (name, len(params), len(argtypes))
            assert _bound_kind(restype) == returns, (name, restype, returns)
            for i, (ctype, want) in enumerate(zip(argtypes, params)):
                assert _bound_kind(ctype) == want, (name, i, ctype, want)
    assert not set(_lib.SIGNATURES) & set(_lib.EXPERIMENT_SIGNATURES)


def test_experiments_library_is_opt_in_and_reference_counted():
    """product code binds libcnrma_hip.so only; `_lib.experiments(True, who)` routes the process's calls through
    libcnrma_hip_exp.so until every `who` has let go (sparse.conv_tuning / rma.dense_tuning / tests are such users)"""
    from cnrma_amd import _lib
    assert not _lib.experiments_active()
    prod = _lib.load()
    assert not hasattr(prod, "cnrma_debug_conv_tuning") and not hasattr(prod, "cnrma_debug_dense_tuning")
    try:
        _lib.experiments(True, "a")
        _lib.experiments(True, "b")
        exp = _lib.load()
        assert exp is not prod and hasattr(exp, "cnrma_debug_conv_tuning") and hasattr(exp, "cnrma_sparse_conv_go_f16x3")
        assert _lib.load(experiments=False) is prod
        _lib.experiments(False, "a")
        assert _lib.experiments_active() and _lib.load() is exp          # "b" still holds it
        _lib.experiments(False, "b")
        assert not _lib.experiments_active() and _lib.load() is prod
    finally:
        _lib.experiments(False, "a")
        _lib.experiments(False, "b")


def test_product_path_fails_loudly_without_gpu():
    from cnrma_amd import _lib, rma
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.CnrmaError):
        rma.to_nhwc(torch.zeros(1, 4, 2, 2))
