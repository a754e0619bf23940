"""Host-side tests of the TSDF fusion (cnrma_amd.fusion): the oracle tests/fusion_oracle.py against the two fixtures recorded from
the reference's TSDFFusion on the CPU (tests/golden/make_golden_fusion.py), the C-ABI declarations, the TSDF container's attribute
volumes, and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import fusion_oracle as FO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnrma_tsdf_fuse_f32", "cnrma_tsdf_fuse_finish_f32")


def load_fixture(golden_dir, name):
    with np.load(os.path.join(golden_dir, f"tsdf_fusion_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    fx["dims"] = tuple(int(n) for n in fx["dims"])
    fx["voxel_size"] = fx["voxel_size"].item()
    fx["origin"] = tuple(float(o) for o in fx["origin"])
    return fx


def oracle_of_fixture(fx, history=False):
    color = torch.from_numpy(fx["color"]) if "color" in fx else None
    label = torch.from_numpy(fx["label"]) if "label" in fx else None
    return FO.fuse(fx["dims"], fx["voxel_size"], fx["origin"], torch.from_numpy(fx["proj"]), torch.from_numpy(fx["depth"]), color, label,
                   trunc_ratio=fx["trunc_ratio"].item(), history=history)


@pytest.mark.parametrize("name", ["general", "edges"])
def test_oracle_equals_the_reference_fixture(golden_dir, name):
    fx = load_fixture(golden_dir, name)
    s = oracle_of_fixture(fx)
    assert torch.equal(s["tsdf"], torch.from_numpy(fx["tsdf_vol"])) and torch.equal(s["weight"], torch.from_numpy(fx["weight_vol"]))
    assert np.array_equal(s["tsdf"].numpy().view(np.uint32), fx["tsdf_vol"].view(np.uint32))           # -0.0 and NaN payloads too
    assert torch.equal(s["color"], torch.from_numpy(fx["color_vol"]))
    t, c = FO.finish(s)
    assert torch.equal(t.view(fx["dims"]), torch.from_numpy(fx["out_tsdf"]))
    assert torch.equal(c.view((3,) + fx["dims"]), torch.from_numpy(fx["out_color"]))
    if name == "edges":
        assert torch.equal(s["label"], torch.from_numpy(fx["label_vol"]))
        assert torch.equal(s["label"].view(fx["dims"]), torch.from_numpy(fx["out_label"]))


def test_fixtures_hold_the_named_cases(golden_dir):
    """what the generator asserted when it wrote the edge fixture, from the committed file"""
    fx = load_fixture(golden_dir, "edges")
    states = oracle_of_fixture(fx, history=True)
    world = FO.world_points(fx["dims"], fx["voxel_size"], fx["origin"])
    P = torch.from_numpy(fx["proj"])
    q = FO.matmul_fma_chain(P[0], world)
    assert int(((q[0] / q[2]) % 1 == 0.5).sum()) == 192                                 # exact .5 ties in px
    assert int((FO.matmul_fma_chain(P[1], world)[2] == 0).sum()) == 192                 # pz == 0
    parked = (states[2]["weight"] == 0) & (states[2]["tsdf"] == -1)
    assert parked.any() and (parked & (states[3]["tsdf"] != -1)).any()                  # dist == -1 at weight 0, then overwritten
    assert ((states[0]["label"] >= 0) & (states[3]["label"] != states[0]["label"])).any()
    assert len(fx["depth"]) == 4 and fx["depth"].shape[1:] == (8, 12)
    for name in ("general", "edges"):
        assert os.path.getsize(os.path.join(golden_dir, f"tsdf_fusion_{name}.npz")) < 1000000


def test_entry_points_declared():
    from cnrma_amd import _lib
    assert _lib.ABI_VERSION == 7
    header = open(os.path.join(ROOT, "include", "cnrma.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m is not None, f"{name} is not declared in include/cnrma.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert "tsdf.py:353-474" in header
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "fusion.hip" in makefile and re.search(r"kernel_resources\.py --check fusion\.resources\.txt fusion_", makefile)


def test_tsdf_attribute_roundtrip(tmp_path):
    from projects.mvsdetection.datasets.tsdf import TSDF
    vol = torch.rand(5, 4, 3) * 2 - 1
    attrs = {"color": torch.rand(3, 5, 4, 3) * 255, "instance": torch.randint(-1, 40, (5, 4, 3))}
    t = TSDF(0.04, torch.tensor([[0.1, 0.2, 0.3]]), vol, attribute_vols=attrs)
    t.save(str(tmp_path / "a.npz"))
    with np.load(str(tmp_path / "a.npz")) as z:
        assert sorted(z.files) == ["color", "instance", "origin", "tsdf", "voxel_size"]
    u = TSDF.load(str(tmp_path / "a.npz"))
    assert torch.equal(u.tsdf_vol, vol) and sorted(u.attribute_vols) == ["color", "instance"]
    assert torch.equal(u.attribute_vols["color"], attrs["color"]) and torch.equal(u.attribute_vols["instance"], attrs["instance"])
    assert u.attribute_vols["instance"].dtype == torch.int64
    assert u.to("cpu") is u and torch.equal(u.attribute_vols["color"], attrs["color"])
    # without attributes: the same three keys as ever, and an empty dict after loading
    p = TSDF(0.04, torch.zeros(1, 3), vol)
    assert p.attribute_vols == {}
    p.save(str(tmp_path / "p.npz"))
    with np.load(str(tmp_path / "p.npz")) as z:
        assert sorted(z.files) == ["origin", "tsdf", "voxel_size"]
    assert TSDF.load(str(tmp_path / "p.npz")).attribute_vols == {}


def test_bad_arguments_raise_before_the_library_is_needed():
    """shape checks come first: they raise ValueError on a machine without a device (the volumes may live on the CPU until the
    first launch, which then refuses them)"""
    from cnrma_amd.fusion import TSDFFusion
    with pytest.raises(ValueError):
        TSDFFusion((4, 4), 0.04, (0, 0, 0), device="cpu")
    with pytest.raises(ValueError):
        TSDFFusion((2048, 2048, 512), 0.04, (0, 0, 0), device="cpu")                    # 2^31 voxels
    f = TSDFFusion((4, 3, 2), 0.04, (0, 0, 0), device="cpu", color=True, label=True)
    assert f.tsdf_vol.eq(1).all() and f.weight_vol.eq(0).all() and f.color_vol.eq(0).all() and f.label_vol.eq(-1).all()
    assert f.label_vol.dtype == torch.int32 and f.color_vol.shape == (3, 24)
    P, d, c, l = torch.zeros(3, 4), torch.ones(6, 8), torch.zeros(3, 6, 8), torch.zeros(6, 8, dtype=torch.long)
    bad = [
        (torch.zeros(4, 4), d, c, l),                     # not a 3x4 projection
        (torch.zeros(12), d, c, l),
        (P, torch.ones(2, 6, 8), c, l),                   # one projection, a batch of depths
        (torch.zeros(2, 3, 4), d, c, l),                  # a batch of projections, one depth
        (torch.zeros(2, 3, 4), torch.ones(3, 6, 8), torch.zeros(3, 3, 6, 8), torch.zeros(3, 6, 8)),      # V differs
        (P, d, None, l),                                  # colour volume without a colour image
        (P, d, c, None),                                  # label volume without a label image
        (P, d, torch.zeros(3, 6, 9), l),                  # W differs
        (P, d, torch.zeros(4, 6, 8), l),                  # four colour planes
        (P, d, c, torch.zeros(5, 8)),                     # H differs
        (torch.zeros(2, 3, 4), torch.ones(2, 6, 8), c, torch.zeros(2, 6, 8)),                            # colour not batched
    ]
    for args in bad:
        with pytest.raises(ValueError):
            f.integrate(*args)
    assert f.tsdf_vol.eq(1).all() and f.weight_vol.eq(0).all()
