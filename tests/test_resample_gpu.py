"""GPU tests of the TSDF resampling (cnrma_amd.resample / csrc/resample.hip).  The pinned behaviour is TSDF.transform on the CPU: the
four fixtures recorded from it (tests/golden/make_golden_resample.py) and, where no fixture exists, tests/resample_oracle.py, which
the generator asserted to equal it bit for bit.  Every comparison is torch.equal -- float volumes are compared as their bit
patterns, so that -0.0 / +0.0 count as well -- with no tolerance and no excluded voxel."""
import math
import random

import numpy as np
import pytest
import torch

import resample_oracle as RO
from test_resample_cpu import FIXTURES, bits, fixture_positions, fixture_tsdf, load_fixture

pytestmark = pytest.mark.gpu
CANARY_F, CANARY_I, PAD = -12345.5, -77, 96


def rot_z(angle, t=(0.0, 0.0, 0.0)):
    T = torch.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = math.cos(angle), -math.sin(angle), math.sin(angle), math.cos(angle)
    T[:3, 3] = torch.tensor(t)
    return T


def random_volume(dims, seed, lo=-1.3, hi=1.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(dims, generator=g) * (hi - lo) + lo).clamp(-1, 1)


def raw(entry, src, src_origin, vs, T, dst_dim, dst_origin, device, fill=None):
    """one of the three entry points through the C ABI, its output inside a larger, canary-filled buffer -> the output (CPU)"""
    from cnrma_amd._lib import call, ptr, stream
    integer = entry.endswith("i64")
    lead = tuple(src.shape[:-3])
    X, Y, Z = src.shape[-3:]
    n = math.prod(lead + tuple(dst_dim))
    buf = torch.full((n + 2 * PAD,), CANARY_I if integer else CANARY_F, dtype=torch.int64 if integer else torch.float32, device=device)
    out = buf[PAD:PAD + n]
    dev = [torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(device) for t in (src_origin, T[:3], dst_origin)]
    s = src.to(device).contiguous()
    args = [ptr(s)] + ([] if entry == "cnrma_tsdf_resample_f32" else [lead[0] if lead else 1])
    args += [X, Y, Z, ptr(dev[0]), float(vs), ptr(dev[1]), ptr(dev[2]), *dst_dim]
    if integer:
        args += [0 if fill is None else fill, 0 if fill is None else 1]
    call(entry, *args, ptr(out), stream())
    torch.cuda.synchronize()
    canary = CANARY_I if integer else CANARY_F
    assert bool((buf[:PAD] == canary).all()) and bool((buf[PAD + n:] == canary).all()), "a canary beside the volume was overwritten"
    return out.cpu().view(lead + tuple(dst_dim))


def same(got, want):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.dtype == torch.float32:
        assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.numel()} voxels differ"
    else:
        assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} voxels differ"


# ---------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_resample_tsdf(device, golden_dir, name):
    from cnrma_amd.resample import resample_tsdf
    fx = load_fixture(golden_dir, name)
    src = fixture_tsdf(fx, device)
    T = torch.from_numpy(fx["transform"])
    for out in (resample_tsdf(src, T, fx["dst_dim"], fx["dst_origin"]), src.transform_device(T[:3], list(fx["dst_dim"]), list(fx["dst_origin"]))):
        assert out.tsdf_vol.is_cuda and out.voxel_size == fx["voxel_size"]
        assert torch.equal(out.origin.cpu(), torch.tensor(fx["dst_origin"], dtype=torch.float32).view(1, 3))
        same(out.tsdf_vol, torch.from_numpy(fx["out"]))
        assert sorted(out.attribute_vols) == sorted(k[4:] for k in fx if k.startswith("out_"))
        for key, vol in out.attribute_vols.items():
            assert vol.is_cuda
            same(vol, torch.from_numpy(fx["out_" + key]))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_entry_points(device, golden_dir, name):
    fx = load_fixture(golden_dir, name)
    geo = (fx["src_origin"], fx["voxel_size"], torch.from_numpy(fx["transform"]), fx["dst_dim"], fx["dst_origin"], device)
    same(raw("cnrma_tsdf_resample_f32", torch.from_numpy(fx["src"]), *geo), torch.from_numpy(fx["out"]))
    if name == "attrs":
        same(raw("cnrma_tsdf_resample_attr_f32", torch.from_numpy(fx["attr_color"]), *geo), torch.from_numpy(fx["out_color"]))
        same(raw("cnrma_tsdf_resample_attr_i64", torch.from_numpy(fx["attr_instance"]), *geo), torch.from_numpy(fx["out_instance"]))
        same(raw("cnrma_tsdf_resample_attr_i64", torch.from_numpy(fx["attr_semseg"]), *geo, fill=-1), torch.from_numpy(fx["out_semseg"]))
        # several integer channels in one launch, and a fill other than -1
        two = torch.stack((torch.from_numpy(fx["attr_instance"]), torch.from_numpy(fx["attr_semseg"])))
        want = RO.resample_int(two, fixture_positions(fx), fill=7)
        same(raw("cnrma_tsdf_resample_attr_i64", two, *geo, fill=7), want)


# ---------------------------------------------------------------------------------------------------- sizes and edge geometry
@pytest.fixture(scope="module")
def small_source():
    """14x11x9 voxels of 0.04 m with colour and labels; read under a rotation that leaves border, band and plain voxels"""
    g = torch.Generator().manual_seed(21)
    return dict(src=random_volume((14, 11, 9), 20), color=torch.rand((3, 14, 11, 9), generator=g) * 255,
                label=torch.randint(1, 50, (14, 11, 9), generator=g), origin=(0.1, -0.2, 0.05), vs=0.04,
                T=rot_z(0.35, (0.22, -0.13, 0.1)))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
@pytest.mark.parametrize("axis", [0, 2])
def test_output_sizes_around_a_wave_and_a_block(device, small_source, n, axis):
    """(n,1,1) walks along x, (1,1,n) along z: n voxels, the last wave and the last block partly filled; the buffers are canaried"""
    sm = small_source
    dst_dim = [1, 1, 1]
    dst_dim[axis] = n
    T = sm["T"].clone()
    T[:3, :3] *= min(1.0, 12.0 / n)                  # any 3x4 map is legal: shorter steps keep a long run inside the source
    dst_origin = (-0.05, 0.03, 0.02)
    pos = RO.positions(sm["src"].shape, sm["origin"], sm["vs"], T, dst_dim, dst_origin)
    if n >= 63:
        assert 0 < int(pos["border"].sum()) < n
    geo = (sm["origin"], sm["vs"], T, dst_dim, dst_origin, device)
    same(raw("cnrma_tsdf_resample_f32", sm["src"], *geo), RO.resample_volume(sm["src"], pos))
    same(raw("cnrma_tsdf_resample_attr_f32", sm["color"], *geo), RO.resample_float(sm["color"], pos))
    same(raw("cnrma_tsdf_resample_attr_i64", sm["label"], *geo, fill=-1), RO.resample_int(sm["label"], pos, fill=-1))


def test_smallest_source(device):
    src = torch.tensor([[[0.5, -0.25], [1.0, 0.75]], [[-1.0, 0.125], [-0.5, 0.0]]])
    T = rot_z(0.3, (0.01, 0.005, -0.01))
    pos = RO.positions((2, 2, 2), (0, 0, 0), 0.04, T, (5, 6, 7), (-0.06, -0.05, -0.04))
    want = RO.resample_volume(src, pos)
    assert 0 < int(pos["border"].sum()) < pos["border"].numel()
    same(raw("cnrma_tsdf_resample_f32", src, (0, 0, 0), 0.04, T, (5, 6, 7), (-0.06, -0.05, -0.04), device), want)


def test_output_outside_the_source_is_all_ones(device):
    src = random_volume((10, 9, 8), 1, -0.9, 0.9)
    T = torch.eye(4)
    T[0, 3] = 10.0
    got = raw("cnrma_tsdf_resample_f32", src, (0, 0, 0), 0.04, T, (9, 7, 11), (0, 0, 0), device)
    assert bool((got == 1).all())
    same(got, RO.resample_volume(src, RO.positions(src.shape, (0, 0, 0), 0.04, T, (9, 7, 11), (0, 0, 0))))


def test_output_inside_the_band(device):
    src = random_volume((20, 18, 16), 2, -0.9, 0.9)                                 # |tsdf| < 1 everywhere
    T = rot_z(0.2, (0.3, 0.2, 0.1))
    pos = RO.positions(src.shape, (0, 0, 0), 0.04, T, (7, 6, 9), (0, 0, 0))
    assert not pos["border"].any() and bool((RO.nearest(src[None], pos).abs() < 1).all())
    same(raw("cnrma_tsdf_resample_f32", src, (0, 0, 0), 0.04, T, (7, 6, 9), (0, 0, 0), device), RO.resample_volume(src, pos))


def test_waves_with_some_lanes_in_the_band_or_on_the_border(device):
    """z-runs of 64 voxels = one wave each, crossing from outside the source through a slab of +-1 (no band) into a band slab:
    waves mixed in the border test, waves mixed in the band test, waves without a band lane and waves wholly on the border"""
    src = random_volume((12, 10, 40), 4, -0.9, 0.9)
    src[:, :, :20] = torch.where(src[:, :, :20] > 0, 1.0, -1.0)
    src[6:] = 1.0                                                                   # a half without any band voxel
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.01, 0.013, -0.6])
    dst_dim, vs = (16, 3, 64), 0.04
    pos = RO.positions(src.shape, (0, 0, 0), vs, T, dst_dim, (-0.08, 0.1, 0.0))
    border = pos["border"].view(-1, 64)
    band = (~pos["border"] & (RO.nearest(src[None], pos)[0].abs() < 1)).view(-1, 64)
    mixed = lambda m: int((m.any(1) & ~m.all(1)).sum())
    assert mixed(border) > 0 and mixed(band) > 0 and int(border.all(1).sum()) > 0 and int((~border.all(1) & ~band.any(1)).sum()) > 0
    same(raw("cnrma_tsdf_resample_f32", src, (0, 0, 0), vs, T, dst_dim, (-0.08, 0.1, 0.0), device), RO.resample_volume(src, pos))


def test_layouts_and_dtypes_are_converted(device):
    from cnrma_amd.resample import resample_tsdf
    from projects.mvsdetection.datasets.tsdf import TSDF
    base = random_volume((9, 12, 10), 6)
    color = torch.rand(3, 9, 12, 10, generator=torch.Generator().manual_seed(1)) * 255            # stored z-major, like base
    label = torch.randint(1, 30, (10, 12, 9), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    origin = torch.tensor([[0.1, 0.0, -0.1]])
    T = rot_z(-0.25, (0.15, 0.2, 0.0))
    src = TSDF(0.04, origin.to(device).double(), base.to(device).double().permute(2, 1, 0),           # fp64, non-contiguous
               dict(color=color.to(device).double().permute(0, 3, 2, 1), instance=label.to(device)))
    assert not src.tsdf_vol.is_contiguous() and not src.attribute_vols["color"].is_contiguous()
    out = resample_tsdf(src, T.double(), (8, 8, 8), (0, 0, 0))
    ref = TSDF(0.04, origin, base.permute(2, 1, 0).contiguous(),
               dict(color=color.permute(0, 3, 2, 1).contiguous(), instance=label.long()))
    vol, attrs = RO.resample_tsdf_oracle(ref, T, (8, 8, 8), (0, 0, 0))
    same(out.tsdf_vol, vol)
    assert out.attribute_vols["color"].dtype == torch.float64 and out.attribute_vols["instance"].dtype == torch.int32
    same(out.attribute_vols["color"].float(), attrs["color"])
    same(out.attribute_vols["instance"].long(), attrs["instance"])


def test_source_dimensions_below_two_are_refused(device):
    from cnrma_amd._lib import CnrmaError
    from cnrma_amd.resample import resample_tsdf
    from projects.mvsdetection.datasets.tsdf import TSDF
    for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
        with pytest.raises(ValueError):
            resample_tsdf(TSDF(0.04, torch.zeros(1, 3, device=device), torch.zeros(shape, device=device)))
        with pytest.raises(CnrmaError, match="invalid argument"):
            raw("cnrma_tsdf_resample_f32", torch.zeros(shape), (0, 0, 0), 0.04, torch.eye(4), (4, 4, 4), (0, 0, 0), device)


def test_defaults_behave_as_on_the_host(device):
    """transform=None, voxel_dim=None, origin=None: the identity into the source's own grid.  Every product of the matrix row is
    then exact, so the host's transform() gives the same bits whatever order its matrix product sums in"""
    from cnrma_amd.resample import resample_tsdf
    from projects.mvsdetection.datasets.tsdf import TSDF
    vol, origin = random_volume((11, 13, 6), 8), torch.tensor([[0.3, -0.7, 0.2]])
    host = TSDF(0.04, origin, vol).transform()
    out = resample_tsdf(TSDF(0.04, origin.to(device), vol.to(device)))
    same(out.tsdf_vol, host.tsdf_vol)
    assert torch.equal(out.origin.cpu(), host.origin) and out.voxel_size == host.voxel_size
    same(out.tsdf_vol, RO.resample_tsdf_oracle(TSDF(0.04, origin, vol))[0])
    # each default on its own
    moved = resample_tsdf(TSDF(0.04, origin.to(device), vol.to(device)), origin=[0.34, -0.7, 0.2], voxel_dim=[5, 4, 3])
    same(moved.tsdf_vol, TSDF(0.04, origin, vol).transform(origin=[0.34, -0.7, 0.2], voxel_dim=[5, 4, 3]).tsdf_vol)


def test_full_size_volume(device):
    """the training shape of the issue: 230x210x90 into 192x192x80 under a rotation about z"""
    from cnrma_amd.resample import resample_tsdf
    from projects.mvsdetection.datasets.tsdf import TSDF
    dims, nd, vs = (230, 210, 90), (192, 192, 80), 0.04
    src = random_volume(dims, 12)
    src[:, :, 40:] = 1.0                                                            # free space above: waves without a band lane
    origin = torch.tensor([[-1.2, 0.4, -0.1]])
    c_src, c_dst = origin[0] + 0.5 * vs * torch.tensor(dims), 0.5 * vs * torch.tensor(nd)
    T = rot_z(0.6)
    T[:3, 3] = c_src - T[:3, :3] @ c_dst
    out = resample_tsdf(TSDF(vs, origin.to(device), src.to(device)), T, nd, (0, 0, 0))
    pos = RO.positions(dims, origin, vs, T, nd, (0, 0, 0))
    assert 0.02 < float(pos["border"].float().mean()) < 0.9
    same(out.tsdf_vol, RO.resample_volume(src, pos))


# ---------------------------------------------------------------------------------------------------- the loading pipeline
@pytest.fixture(scope="module")
def dataset_root(tmp_path_factory):
    from cnrma_amd import synth
    root = str(tmp_path_factory.mktemp("scannet_like_resample"))
    return root, synth.write_scannet_like(root, n_scenes=1, V=4, dims=(48, 48, 24), img_hw=(60, 80))


def run_pipeline(dataset_root, space_transform, test_mode, device, seed=11):
    """one sample through the loading pipeline and data_converter -> (tsdf_list, the sample's tsdf_dict, projection)"""
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.models.multiview_base import MultiViewBase
    from projects.mvsdetection.registry import DATASETS
    root, ann = dataset_root
    pipe = [dict(type="AtlasResizeImage", size=(80, 60)), dict(type="AtlasToTensor"), space_transform,
            dict(type="AtlasIntrinsicsPoseToProjection"), dict(type="AtlasCollectData")]
    ds = DATASETS.build(dict(type="AtlasScanNetDataset", data_root=root, ann_file=ann, classes=["a", "b", "c", "d"], pipeline=pipe,
                             test_mode=test_mode, num_frames=3, voxel_size=0.04, select_type="unit"))
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    s = ds[0]
    tsdf_dict = s["tsdf_dict"].data
    data = MultiViewBase.data_converter(None, dict(projection=[s["projection"].data.to(device)], tsdf_dict=[dict(tsdf_dict)]))
    assert "tsdf_dict" not in data
    return data["tsdf_list"], tsdf_dict, s["projection"].data


@pytest.mark.parametrize("space_transform", [
    dict(type="AtlasTestTransformSpaceRecon", voxel_dim=[48, 48, 24], origin=[0, 0, 0]),
    dict(type="AtlasTransformSpaceDetection", voxel_dim=[40, 56, 24], origin=[0, 0, 0], test=True, mode="origin"),
    dict(type="AtlasTransformSpaceDetection", voxel_dim=[56, 40, 16], origin=[0, 0, 0], test=True, mode="middle"),
])
def test_pipeline_translations_equal_the_host_path(device, dataset_root, space_transform):
    """the test-time space transforms are pure translations: one non-zero product per row, exact in any summation order, so the
    live host path is a valid pin"""
    from projects.mvsdetection.datasets.tsdf import TSDF, DeferredTSDF
    host, host_dict, host_proj = run_pipeline(dataset_root, dict(space_transform, tsdf_resample="host"), True, device)
    dev, dev_dict, dev_proj = run_pipeline(dataset_root, dict(space_transform, tsdf_resample="device"), True, device)
    assert all(type(v) is TSDF for v in host_dict.values()) and all(type(v) is DeferredTSDF for v in dev_dict.values())
    assert torch.equal(host_proj, dev_proj) and sorted(host) == sorted(dev) == ["tsdf_gt_004", "tsdf_gt_008", "tsdf_gt_016"]
    for key in host:
        assert dev[key].is_cuda and dev[key].shape == host[key].shape and dev[key].dim() == 5
        same(dev[key], host[key])
        assert 0 < int((host[key] != 1).sum())


def test_pipeline_random_rotation_equals_the_oracle(device, dataset_root):
    """the training augmentation: both modes draw the same rotation and crop; the device result equals the oracle bit for bit.
    Against the live host path only the number of differing voxels is reported: its matrix product sums in the BLAS's order"""
    space = dict(type="AtlasRandomTransformSpaceRecon", voxel_dim=[32, 40, 16], random_rotation=True, random_translation=True,
                 paddingXY=0.2, paddingZ=0.1)
    host, _, host_proj = run_pipeline(dataset_root, dict(space, tsdf_resample="host"), False, device)
    dev, dev_dict, dev_proj = run_pipeline(dataset_root, dict(space, tsdf_resample="device"), False, device)
    assert torch.equal(host_proj, dev_proj)
    for key, d in dev_dict.items():
        T = d.transform_matrix
        assert float(T[0, 1].abs()) > 1e-3                                          # a rotation was drawn
        pos = RO.positions(d.source.tsdf_vol.shape, d.source.origin, d.voxel_size, T, d.voxel_dim, d.new_origin)
        want = RO.resample_volume(d.source.tsdf_vol, pos)
        same(dev[key][0, 0], want)
        assert 0 < int((want != 1).sum())
        differ = int((bits(dev[key]) != bits(host[key])).sum())
        print(f"{key}: {differ} of {want.numel()} voxels differ between the device run and the live host run")


def test_raymarching_train_step_with_deferred_volumes(device, tmp_path):
    """train_step of the registered detector fed what a tsdf_resample="device" pipeline hands over: data_converter resolves the
    DeferredTSDF on the GPU and the detector marches on the result"""
    import os
    import runpy
    import projects.mvsdetection  # noqa: F401
    from cnrma_amd import synth
    from projects.mvsdetection.datasets.pipelines.atlas_transforms import transform_space
    from projects.mvsdetection.datasets.tsdf import TSDF, DeferredTSDF
    from projects.mvsdetection.registry import build_model
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sc = synth.make_scene("tiny", seed=6)
    C = sc["features"].shape[2]
    cfg = runpy.run_path(os.path.join(root, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))
    m = dict(cfg["model"])
    m.update(backbone2d=None, feature_2d=None, backbone_3d=None, tsdf_head=None)      # hot path only: features come in
    m.update(save_path=str(tmp_path / "r"), voxel_dim_test=list(sc["dims"]), voxel_dim_train=list(sc["dims"]), max_points=None,
             use_feature_transform=False, detection_backbone=dict(type="FCAF3DBackbone", in_channels=C, depth=14))
    torch.manual_seed(2)
    np.random.seed(3)
    model = build_model(m)
    model.detection_backbone.init_weights()
    model.detection_head.init_weights()
    model = model.to(device).train()
    # the scene's volume stored one voxel off the detector's grid: the space transform is the translation that brings it back
    sample = dict(extrinsics=[], tsdf_dict={"tsdf_gt_004": TSDF(0.04, torch.tensor([[0.04, 0.04, 0.04]]), sc["tsdf"][0, 0].clone())})
    sample = transform_space(sample, torch.eye(4), list(sc["dims"]), [0, 0, 0], resample="device")
    assert type(sample["tsdf_dict"]["tsdf_gt_004"]) is DeferredTSDF
    dims = np.array(sc["dims"], dtype=np.float32) * 0.04
    boxes = torch.tensor([[0.35 * dims[0], 0.4 * dims[1], 0.1 * dims[2], 0.5, 0.4, 0.5, 0.0],
                          [0.65 * dims[0], 0.6 * dims[1], 0.2 * dims[2], 0.4, 0.6, 0.4, 0.0]], device=device)
    data = dict(features=[sc["features"][:, 0].to(device)], projection=[sc["projection"][:, 0].to(device)],
                offset=[torch.zeros(3, device=device)], gt_bboxes_3d=[boxes], gt_labels_3d=[torch.tensor([1, 3], device=device)],
                tsdf_dict=[sample["tsdf_dict"]])
    out = model.train_step(dict(data), None)
    assert set(out["log_vars"]) >= {"loss_centerness", "loss_bbox", "loss_cls", "total_loss"}
    assert torch.isfinite(out["loss"]) and all(math.isfinite(v) for v in out["log_vars"].values())
    assert model.points_detection[0].shape[0] > 0 and model._last_tsdf.is_cuda
    d = sample["tsdf_dict"]["tsdf_gt_004"]
    pos = RO.positions(d.source.tsdf_vol.shape, d.source.origin, 0.04, torch.eye(4), d.voxel_dim, [0, 0, 0])
    same(model._last_tsdf[0, 0], RO.resample_volume(d.source.tsdf_vol, pos))
