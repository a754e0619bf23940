"""Host-side tests of the TSDF resampling (cnrma_amd.resample): the oracle tests/resample_oracle.py against the four fixtures
recorded from TSDF.transform on the CPU (tests/golden/make_golden_resample.py), the C-ABI declarations, the build rule, and the
deferred resampling of the loading pipeline, which needs no device until the detector resolves it."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import resample_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnrma_tsdf_resample_f32", "cnrma_tsdf_resample_attr_f32", "cnrma_tsdf_resample_attr_i64")
FIXTURES = ("general", "ties", "oblique", "attrs")


def load_fixture(golden_dir, name):
    with np.load(os.path.join(golden_dir, f"tsdf_resample_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    fx["dst_dim"] = tuple(int(n) for n in fx["dst_dim"])
    fx["voxel_size"] = fx["voxel_size"].item()
    fx["src_origin"] = tuple(float(o) for o in fx["src_origin"])
    fx["dst_origin"] = tuple(float(o) for o in fx["dst_origin"])
    return fx


def fixture_tsdf(fx, device="cpu"):
    """the fixture's source as a TSDF (attribute volumes included)"""
    from projects.mvsdetection.datasets.tsdf import TSDF
    attrs = {k[5:]: torch.from_numpy(v).to(device) for k, v in fx.items() if k.startswith("attr_")}
    return TSDF(fx["voxel_size"], torch.tensor(fx["src_origin"], dtype=torch.float32, device=device).view(1, 3),
                torch.from_numpy(fx["src"]).to(device), attrs)


def fixture_positions(fx):
    return RO.positions(fx["src"].shape, fx["src_origin"], fx["voxel_size"], torch.from_numpy(fx["transform"]), fx["dst_dim"],
                        fx["dst_origin"])


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_fixture(golden_dir, name):
    fx = load_fixture(golden_dir, name)
    vol, attrs = RO.resample_tsdf_oracle(fixture_tsdf(fx), torch.from_numpy(fx["transform"]), fx["dst_dim"], fx["dst_origin"])
    want = torch.from_numpy(fx["out"])
    assert vol.shape == want.shape and torch.equal(bits(vol), bits(want)), int((bits(vol) != bits(want)).sum())
    assert sorted(attrs) == sorted(k[4:] for k in fx if k.startswith("out_"))
    for key, got in attrs.items():
        want = torch.from_numpy(fx["out_" + key])
        assert got.dtype == want.dtype and got.shape == want.shape
        assert torch.equal(bits(got), bits(want)) if got.dtype == torch.float32 else torch.equal(got, want)


def test_fixtures_hold_the_named_cases(golden_dir):
    """what the generator asserted when it wrote the fixtures, from the committed files"""
    for name in FIXTURES:
        assert os.path.getsize(os.path.join(golden_dir, f"tsdf_resample_{name}.npz")) < 1000000
    # general: the shapes of the issue, a rotation about z, a live band and a border that is neither empty nor everything
    fx = load_fixture(golden_dir, "general")
    assert fx["src"].shape == (64, 50, 23) and fx["dst_dim"] == (48, 40, 24) and fx["voxel_size"] == 0.08
    T = fx["transform"]
    assert np.allclose(T[:2, :2], [[np.cos(0.7), -np.sin(0.7)], [np.sin(0.7), np.cos(0.7)]], atol=1e-6) and T[2, 2] == 1
    assert np.abs(T[:3, 3]).min() > 0 and np.abs(fx["src"]).max() == 1.0
    pos = fixture_positions(fx)
    near = RO.nearest(torch.from_numpy(fx["src"])[None], pos)[0]
    band, border = (~pos["border"] & (near.abs() < 1)).float().mean(), pos["border"].float().mean()
    assert band >= 0.10 and 0.10 <= border <= 0.90
    # ties: a pure translation by half a voxel; exact .5 ties in s, also off the border; and no nearest index outside the volume
    # while |n| < 1 (the generator shows that none can be built)
    fx = load_fixture(golden_dir, "ties")
    assert np.array_equal(fx["transform"][:3, :3], np.eye(3)) and np.all(fx["transform"][:3, 3] == 0.5 * fx["voxel_size"])
    assert all(d % 2 == 0 for d in fx["src"].shape)
    pos = fixture_positions(fx)
    tie = (pos["s"] - torch.floor(pos["s"])) == 0.5
    assert int(tie.sum()) == 620 and int((tie & ~pos["border"]).sum()) == 347
    r = torch.round(pos["s"])
    assert not (((r < 0) | (r >= torch.tensor(fx["src"].shape).view(3, 1))).any(0) & ~pos["border"]).any()
    # oblique: nearly every output z-run changes its source x and its source y
    fx = load_fixture(golden_dir, "oblique")
    pos = fixture_positions(fx)
    nx, ny, nz = fx["dst_dim"]
    r = torch.round(pos["s"]).view(3, nx * ny, nz)
    assert float(((r[0].max(1).values != r[0].min(1).values) & (r[1].max(1).values != r[1].min(1).values)).float().mean()) > 0.9
    # attrs: colour with padded corners off the border, instance zero-padded (not filled) on the border, semseg -1 there
    fx = load_fixture(golden_dir, "attrs")
    assert fx["attr_color"].shape == (3, 20, 18, 12) and fx["attr_color"].dtype == np.float32
    assert fx["attr_instance"].dtype == np.int64 and fx["attr_semseg"].dtype == np.int64
    pos = fixture_positions(fx)
    border = pos["border"].view(fx["dst_dim"]).numpy()
    assert (fx["out_semseg"][border] == -1).all() and (fx["out_semseg"][~border] > 0).all()
    assert (fx["out_instance"][border] == 0).any() and (fx["out_instance"] >= 0).all() and (fx["out_instance"][~border] > 0).all()
    f, d = torch.floor(pos["s"]), torch.tensor(fx["src"].shape, dtype=torch.float32).view(3, 1)
    assert int((((f < 0) | (f + 1 >= d)).any(0) & ~pos["border"]).sum()) >= 100


def test_entry_points_declared():
    from cnrma_amd import _lib
    assert _lib.ABI_VERSION == 7
    header = open(os.path.join(ROOT, "include", "cnrma.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", header)
        assert m is not None, f"{name} is not declared in include/cnrma.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert "a17  TSDF resampling" in header and "tsdf.py:112-180" in header


def test_makefile_checks_the_kernels_resources():
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bresample\.hip\b", makefile, re.M) and re.search(r"^EXP_OBJS = .*\bresample\.o\b", makefile, re.M)
    assert re.search(r"-Rpass-analysis=kernel-resource-usage -c \$< -o \$@ 2> resample\.resources\.txt", makefile)
    assert re.search(r"kernel_resources\.py --check resample\.resources\.txt tsdf_resample_", makefile)


def test_bad_arguments_raise_before_the_library_is_needed():
    from cnrma_amd.resample import resample_tsdf
    from projects.mvsdetection.datasets.tsdf import TSDF
    o = torch.zeros(1, 3)
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):                                # the grid is normalised by dim - 1
        with pytest.raises(ValueError):
            resample_tsdf(TSDF(0.04, o, torch.zeros(shape)))
    with pytest.raises(ValueError):
        resample_tsdf(TSDF(0.04, o, torch.zeros(4, 4)))
    t = TSDF(0.04, o, torch.zeros(4, 4, 4))
    with pytest.raises(ValueError):
        resample_tsdf(t, voxel_dim=(2048, 2048, 512))                              # 2^31 voxels
    with pytest.raises(ValueError):
        resample_tsdf(t, voxel_dim=(4, 4))
    with pytest.raises(ValueError):
        resample_tsdf(TSDF(0.04, o, torch.zeros(4, 4, 4), dict(color=torch.zeros(3, 4, 4, 5))))
    with pytest.raises(ValueError):
        resample_tsdf(TSDF(0.04, o, torch.zeros(4, 4, 4), dict(mask_outside=torch.zeros(4, 4, 4, dtype=torch.bool))))
    assert callable(TSDF.transform_device)


# ---------------------------------------------------------------------------------------------------- deferred resampling
def test_deferred_tsdf_reads_as_the_host_transform():
    from projects.mvsdetection.datasets.tsdf import TSDF, DeferredTSDF
    torch.manual_seed(3)
    src = TSDF(0.04, torch.tensor([[0.2, -0.1, 0.3]]), (torch.rand(14, 12, 10) * 2.6 - 1.3).clamp(-1, 1))
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.08, -0.04, 0.12])                                   # a pure translation
    want = src.transform(T, [12, 12, 8], [0, 0, 0])
    d = DeferredTSDF(src, T, [12, 12, 8], [0, 0, 0])
    assert d.voxel_size == want.voxel_size and torch.equal(d.origin, want.origin) and d._host is None
    assert torch.equal(bits(d.tsdf_vol), bits(want.tsdf_vol)) and d.tsdf_vol is d.tsdf_vol
    assert d.attribute_vols == {} and d.device == want.device                     # every other reader: the host TSDF
    assert torch.equal(d.transform().tsdf_vol, want.transform().tsdf_vol)
    with pytest.raises(AttributeError):
        d.no_such_attribute
    e = copy.deepcopy(DeferredTSDF(src, T, [12, 12, 8], None))                     # survives a trip through a worker's pickle
    assert torch.equal(e.origin, src.origin) and torch.equal(e.tsdf_vol, src.transform(T, [12, 12, 8]).tsdf_vol)


def sample(seed=5):
    from projects.mvsdetection.datasets.tsdf import TSDF
    g = torch.Generator().manual_seed(seed)
    vols = {f"tsdf_gt_{vs:03d}": TSDF(0.01 * vs, torch.tensor([[0.3, -0.2, 0.1]]),
                                      (torch.rand(96 // vs, 80 // vs, 64 // vs, generator=g) * 2.6 - 1.3).clamp(-1, 1)) for vs in (4, 8, 16)}
    return dict(extrinsics=[torch.eye(4) + 0.1 * torch.rand(4, 4, generator=g) for _ in range(3)], tsdf_dict=vols)


def test_transform_space_modes_consume_the_rng_alike():
    from projects.mvsdetection.datasets.pipelines.atlas_transforms import AtlasRandomTransformSpaceRecon, transform_space
    from projects.mvsdetection.datasets.tsdf import TSDF, DeferredTSDF
    out, states = {}, {}
    for mode in ("host", "device"):
        torch.manual_seed(17)
        np.random.seed(17)
        t = AtlasRandomTransformSpaceRecon([16, 16, 8], paddingXY=0.2, paddingZ=0.1, tsdf_resample=mode)
        out[mode] = t(sample())
        states[mode] = (torch.get_rng_state(), np.random.get_state()[1].copy())
    assert torch.equal(states["host"][0], states["device"][0]) and np.array_equal(states["host"][1], states["device"][1])
    for a, b in zip(out["host"]["extrinsics"], out["device"]["extrinsics"]):
        assert torch.equal(a, b)
    assert torch.equal(out["host"]["offset"], out["device"]["offset"])
    for key, h in out["host"]["tsdf_dict"].items():
        d = out["device"]["tsdf_dict"][key]
        assert type(h) is TSDF and type(d) is DeferredTSDF
        assert d.voxel_size == h.voxel_size and torch.equal(d.origin, h.origin)
        assert d.voxel_dim == list(h.tsdf_vol.shape) and torch.equal(bits(d.tsdf_vol), bits(h.tsdf_vol))
    with pytest.raises(ValueError):
        transform_space(sample(), torch.eye(4), [16, 16, 8], [0, 0, 0], resample="gpu")


def test_defaults_produce_plain_tsdf_objects():
    import inspect
    import runpy
    from projects.mvsdetection.datasets.pipelines.atlas_transforms import (AtlasRandomTransformSpaceRecon,
                                                                           AtlasTestTransformSpaceRecon, transform_space)
    from projects.mvsdetection.datasets.pipelines.fcaf3d_transforms import AtlasTransformSpaceDetection
    from projects.mvsdetection.datasets.tsdf import TSDF
    assert inspect.signature(transform_space).parameters["resample"].default == "host"
    for t in (AtlasRandomTransformSpaceRecon([16, 16, 8]), AtlasTestTransformSpaceRecon([16, 16, 8], [0, 0, 0]),
              AtlasTransformSpaceDetection([16, 16, 8], test=True)):
        assert t.tsdf_resample == "host"
        torch.manual_seed(0)
        assert all(type(v) is TSDF for v in t(sample())["tsdf_dict"].values())
    # the builders: the default adds no key (the six configs are unchanged), "device" reaches both pipelines
    b = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "_builders.py"))
    for build, args in ((b["recon_pipelines"], ([16, 16, 8], [16, 16, 8])), (b["detection_pipelines"], ([16, 16, 8], [16, 16, 8], "origin"))):
        assert all("tsdf_resample" not in p[2] for p in build(*args))
        assert all(p[2]["tsdf_resample"] == "device" for p in build(*args, tsdf_resample="device"))
