"""Host-side tests of the fusion-volume bounds (cnrma_amd.fusion.scene_bounds): the oracle tests/bounds_oracle.py against the two
fixtures recorded beside the reference's depth_to_world on the CPU (tests/golden/make_golden_bounds.py), the host finish against
np.quantile, the preparation library's C surface (include/cnrma_prep.h), and the argument checks that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import bounds_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F, D, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
PREP_TABLE = {
    "cnrma_prep_abi_version": (I, []),
    "cnrma_prep_bounds_workspace_bytes": (Z, []),
    "cnrma_prep_depth_bounds_f32": (I, [P, P, I, I, I, F, D, D, P, Z, P, P, P]),
}


def load_fixture(golden_dir, name):
    with np.load(os.path.join(golden_dir, f"bounds_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    for k in ("voxel_size", "max_depth", "vol_prcnt", "vol_margin", "n"):
        fx[k] = fx[k].item()
    fx["voxel_dim"] = [int(d) for d in fx["voxel_dim"]]
    return fx


def same(a, b):
    """== on every element (so +0.0 is -0.0), a NaN equal to a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | ((a != a) & (b != b))).all())


@pytest.mark.parametrize("name", ["general", "edge"])
def test_oracle_equals_the_reference_fixture(golden_dir, name):
    fx = load_fixture(golden_dir, name)
    proj, depth = torch.from_numpy(fx["proj"]), torch.from_numpy(fx["depth"])
    # the inverses are pinned as an INPUT: torch.inverse (LAPACK) is not bit-stable across host CPUs, so the recorded ones (computed
    # where the reference ran) are what makes the points comparable bit for bit; this host's own are merely close
    for v in range(len(proj)):
        np.testing.assert_allclose(BO.inverse_projection(proj[v]).numpy(), fx["pinv"][v], rtol=1e-4, atol=1e-5)
    pts = BO.cloud(proj, depth, fx["max_depth"], pinv=torch.from_numpy(fx["pinv"]))
    assert len(pts) == fx["n"] and pts.dtype == np.float32
    origin, dim, q = BO.bounds_of_cloud(pts, fx["voxel_size"], fx["vol_prcnt"], fx["vol_margin"])
    assert np.array_equal(q.view(np.uint32), fx["quantiles"].view(np.uint32))
    assert np.array_equal(origin.numpy().view(np.uint32), fx["origin"].view(np.uint32)) and dim == fx["voxel_dim"]
    values, counts = BO.order_statistics(pts, 1 - fx["vol_prcnt"], fx["vol_prcnt"])
    assert np.array_equal(values.view(np.uint32), fx["values"].view(np.uint32)) and np.array_equal(counts, fx["counts"])


def test_fixtures_hold_the_named_cases(golden_dir):
    """what the generator asserted when it wrote the fixtures, from the committed files"""
    fx = load_fixture(golden_dir, "general")
    d = fx["depth"]
    assert d.shape == (3, 24, 32) and fx["max_depth"] == 3.0
    assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and np.isposinf(d).any() and (d[np.isfinite(d)] > 3.0).any()
    assert fx["n"] == int(((d <= 3.0) & (d != 0)).sum())                       # negative depths are kept
    assert (fx["pinv"][:, 3] != np.array([0, 0, 0, 1], np.float32)).any()       # the inverse's last row is not exactly 0 0 0 1
    fx = load_fixture(golden_dir, "edge")
    assert fx["depth"].shape == (4, 8, 8) and np.array_equal(fx["depth"][:2], fx["depth"][2:]) and fx["n"] == 256
    s = np.sort(BO.cloud(None, torch.from_numpy(fx["depth"]), pinv=torch.from_numpy(fx["pinv"])), axis=0)
    assert (s[0::2] == s[1::2]).all()                                           # every value is a tie
    k, k1 = BO.ranks(256, fx["vol_prcnt"])
    assert (k, k1) == (191, 192) and BO.ranks(256, 1 - fx["vol_prcnt"]) == (63, 64)
    assert s[k, 2] < 0 < 40 < s[k1, 2] and BO.float_key(s[k, 2]) >> 24 != BO.float_key(s[k1, 2]) >> 24
    assert all((s[:, a] < 0).any() and (s[:, a] > 0).any() for a in range(3))
    for name in ("general", "edge"):
        assert os.path.getsize(os.path.join(golden_dir, f"bounds_{name}.npz")) < 100000


def test_float_key_orders_like_the_floats():
    x = np.array([-np.inf, -3.5, -1e-40, 0.0, 1e-40, 1.0, 1.0000001, 7e30, np.inf], np.float32)
    keys = [BO.float_key(v) for v in x]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 200, 256, 1001])
@pytest.mark.parametrize("q", [0.0, 0.005, 1 - .995, 0.25, 0.5, 0.75, .995, 1.0])
def test_host_finish_equals_np_quantile(n, q):
    """the order statistics the device delivers, interpolated by the wrapper's finish, are np.quantile bit for bit"""
    from cnrma_amd.fusion import quantile_finish
    rng = np.random.default_rng(n)
    pts = (rng.standard_normal((n, 3)) * [1, 10, 1e-3]).astype(np.float32)
    values, counts = BO.order_statistics(pts, q, q)
    got = quantile_finish(values[0, :, 0], values[0, :, 1], n, q, counts[1:])
    exp = np.quantile(pts, q, axis=0)
    assert got.dtype == exp.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_host_finish_with_nans_and_infinities():
    from cnrma_amd.fusion import quantile_finish
    pts = np.random.default_rng(1).standard_normal((50, 3)).astype(np.float32)
    pts[7, 1] = np.nan
    pts[3, 2] = np.inf
    pts[4, 2] = -np.inf
    for q in (0.0, 0.3, 1.0):
        values, counts = BO.order_statistics(pts, q, q)
        assert counts.tolist() == [50, 0, 1, 0]
        with np.errstate(invalid="ignore"):
            got, exp = quantile_finish(values[0, :, 0], values[0, :, 1], 50, q, counts[1:]), np.quantile(pts, q, axis=0)
        assert np.isnan(got[1]) and same(got, exp)


def test_prep_signatures_equal_the_hand_typed_table():
    from cnrma_amd import _lib
    assert _lib.PREP_SIGNATURES == PREP_TABLE and list(_lib.PREP_SIGNATURES) == list(PREP_TABLE)
    assert _lib.PREP_ABI_VERSION == 1 and _lib.PREP_CONSTANTS["CNRMA_PREP_EINVAL"] == -22
    assert len(_lib.SIGNATURES) == 128 and _lib.ABI_VERSION == 7                 # the product surface is as it was
    assert not any(name.startswith("cnrma_prep_") for name in list(_lib.SIGNATURES) + list(_lib.EXPERIMENT_SIGNATURES))
    header = open(_lib.PREP_HEADER_PATH).read()
    assert "generate_tsdf.py:82-101" in header and "tsdf.py:77-101" in header
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "kernel_resources.py --check bounds.resources.txt bounds_" in makefile


def test_prep_library_exports_exactly_the_header():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.PREP_LIB_PATH):                                   # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.PREP_LIB_PATH), "-j8", "libcnrma_prep_hip.so"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.PREP_LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}
    assert names == set(PREP_TABLE)
    lib = _lib.load_prep()
    assert lib.cnrma_prep_abi_version() == 1
    nbytes = lib.cnrma_prep_bounds_workspace_bytes()
    assert 0 < nbytes < 1 << 20 and nbytes % 4 == 0
    # the argument checks come before any launch: they answer without a device
    args = dict(V=1, H=2, W=2, q_lo=0.005, q_hi=0.995, ws=nbytes)

    def rc(**kw):
        a = dict(args, **kw)
        return lib.cnrma_prep_depth_bounds_f32(64, 64, a["V"], a["H"], a["W"], np.inf, a["q_lo"], a["q_hi"], 64, a["ws"], 64, 64, None)
    for bad in (dict(V=-1), dict(H=-1), dict(W=-1), dict(V=1 << 11, H=1 << 10, W=1 << 10), dict(H=1 << 16, W=1 << 16), dict(q_lo=-0.1),
                dict(q_hi=1.5), dict(q_lo=float("nan")), dict(ws=nbytes - 4), dict(ws=0)):
        assert rc(**bad) == -22, bad


def test_bad_arguments_raise_before_the_library_is_needed():
    from cnrma_amd.fusion import fuse_scene, scene_bounds
    P3, d = torch.zeros(2, 3, 4), torch.ones(2, 6, 8)
    bad = [
        (torch.zeros(3, 4), torch.ones(6, 8)),            # one view: scene_bounds wants batches
        (torch.zeros(2, 4, 4), d),                        # not 3x4 projections
        (torch.zeros(2, 12), d),
        (P3, torch.ones(3, 6, 8)),                        # V differs
        (P3, torch.ones(2, 48)),                          # depth maps without rows
    ]
    with pytest.raises(ValueError):
        scene_bounds(P3, d, 0.04, pinv=torch.zeros(3, 4, 4))             # one inverse per view
    for args in bad:
        with pytest.raises(ValueError):
            scene_bounds(*args, 0.04)
        with pytest.raises(ValueError):
            fuse_scene(*args)
    for kw in (dict(vol_prcnt=1.5), dict(vol_prcnt=-0.1), dict(voxel_size=0.0)):
        with pytest.raises(ValueError):
            scene_bounds(P3, d, **dict(dict(voxel_size=0.04), **kw))
    with pytest.raises(ValueError):
        fuse_scene(P3, d, batch=0)
