"""GPU tests of the fusion-volume bounds (cnrma_amd.fusion.scene_bounds / fuse_scene, csrc/bounds.hip).  The pinned behaviour is the
reference's host arithmetic on the CPU: the two fixtures recorded beside it (tests/golden/make_golden_bounds.py) and, where no fixture
exists, tests/bounds_oracle.py (which the generator asserted to equal the reference bit for bit) with np.quantile as the judge of the
quantiles.  Origins and quantiles are compared as bit patterns; the order statistics of the C entry point with == (the sign of a zero
is not pinned, a NaN equals a NaN).  No tolerance anywhere."""
import math

import numpy as np
import pytest
import torch

import bounds_oracle as BO
import fusion_oracle as FO
from test_bounds_cpu import load_fixture, same
from test_fusion_gpu import look_at, ring_scene, sphere_scene

pytestmark = pytest.mark.gpu
CANARY_F, CANARY_I, PAD = -12345.5, -77, 96


def bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int32)


def inverses(proj):
    return torch.stack([BO.inverse_projection(p) for p in proj]) if len(proj) else torch.zeros(0, 4, 4)


def raw_bounds(device, pinv, depth, q_lo, q_hi, max_depth=math.inf):
    """cnrma_prep_depth_bounds_f32 through the C ABI with workspace and outputs inside larger, canary-filled buffers
    -> (values [2,3,2] float32, counts [4] int64); the values start as the canary, so untouched ones show"""
    from cnrma_amd import _lib
    from cnrma_amd._lib import call_prep, ptr, stream
    nbytes = _lib.load_prep().cnrma_prep_bounds_workspace_bytes()
    ws = torch.full((nbytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device=device)
    values = torch.full((12 + 2 * PAD,), CANARY_F, device=device)
    counts = torch.full((4 + 2 * PAD,), CANARY_I, dtype=torch.int64, device=device)
    V, H, W = depth.shape
    pinv, depth = pinv.to(device, torch.float32).contiguous(), depth.to(device, torch.float32).contiguous()
    call_prep("cnrma_prep_depth_bounds_f32", ptr(pinv) if pinv.numel() else None, ptr(depth) if depth.numel() else None, V, H, W,
              max_depth, q_lo, q_hi, ws.data_ptr() + PAD, nbytes, values.data_ptr() + 4 * PAD, counts.data_ptr() + 8 * PAD, stream())
    torch.cuda.synchronize()
    assert bool((ws[:PAD] == 0xA5).all()) and bool((ws[-PAD:] == 0xA5).all()), "a canary beside the workspace was overwritten"
    assert bool((values[:PAD] == CANARY_F).all()) and bool((values[-PAD:] == CANARY_F).all()), "a canary beside the values"
    assert bool((counts[:PAD] == CANARY_I).all()) and bool((counts[-PAD:] == CANARY_I).all()), "a canary beside the counts"
    return values[PAD:PAD + 12].cpu().numpy().reshape(2, 3, 2), counts[PAD:PAD + 4].cpu().numpy()


def check_raw(device, proj, depth, vol_prcnt, max_depth=None, pinv=None):
    """the C entry point against the sorted oracle cloud; -> the cloud"""
    pinv = inverses(proj) if pinv is None else pinv
    pts = BO.cloud(proj, depth, max_depth, pinv=pinv)
    exp_values, exp_counts = BO.order_statistics(pts, 1 - vol_prcnt, vol_prcnt)
    values, counts = raw_bounds(device, pinv, depth, 1 - vol_prcnt, vol_prcnt, math.inf if max_depth is None else max_depth)
    assert counts.tolist() == exp_counts.tolist()
    if len(pts):
        assert same(values, exp_values), (values, exp_values)
    else:
        assert bool((values == CANARY_F).all())                          # n == 0: the values are left untouched
    return pts


def check_scene(device, proj, depth, voxel_size=0.04, max_depth=None, vol_prcnt=.995, vol_margin=1.5):
    """scene_bounds against the oracle (np.quantile over the oracle's cloud)"""
    from cnrma_amd.fusion import scene_bounds
    exp_origin, exp_dim, _ = BO.bounds(proj, depth, voxel_size, max_depth, vol_prcnt, vol_margin)
    origin, dim = scene_bounds(proj, depth, voxel_size, max_depth, vol_prcnt, vol_margin, device=device)
    assert origin.dtype == torch.float32 and not origin.is_cuda and tuple(origin.shape) == (3,) and isinstance(dim, list)
    assert torch.equal(bits(origin), bits(exp_origin)), (origin, exp_origin)
    assert dim == exp_dim
    return origin, dim


def fixture_views(golden_dir, name):
    fx = load_fixture(golden_dir, name)
    return fx, torch.from_numpy(fx["proj"]), torch.from_numpy(fx["depth"])


def small_scene(V, H, W, seed):
    """V ring cameras with depths through the volume's range and zero / NaN / inf / negative pixels (test_fusion_gpu.ring_scene)"""
    sc = ring_scene((20, 16, 12), V, H, W, seed)
    return sc["proj"], sc["depth"]


# ---------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", ["general", "edge"])
def test_fixture_through_scene_bounds(device, golden_dir, name):
    """against the recorded result with the recorded inverses (torch.inverse is not bit-stable across host CPUs: the inverses are
    pinned as an input, as in test_rma_gpu), and with this host's own inverses against the oracle on this host"""
    from cnrma_amd.fusion import scene_bounds
    fx, proj, depth = fixture_views(golden_dir, name)
    max_depth = None if math.isinf(fx["max_depth"]) else fx["max_depth"]
    origin, dim = scene_bounds(proj, depth, fx["voxel_size"], max_depth, fx["vol_prcnt"], fx["vol_margin"], device=device,
                               pinv=fx["pinv"])
    assert torch.equal(bits(origin), bits(torch.from_numpy(fx["origin"]))) and dim == fx["voxel_dim"]
    origin, dim = check_scene(device, proj, depth, fx["voxel_size"], max_depth, fx["vol_prcnt"], fx["vol_margin"])
    # inputs already on the device, depth as a strided view, projections as float64 numpy
    wide = torch.zeros(depth.shape[0], depth.shape[1], 2 * depth.shape[2], device=device)
    wide[:, :, ::2] = depth.to(device)
    origin2, dim2 = scene_bounds(proj.double().numpy(), wide[:, :, ::2], fx["voxel_size"], max_depth, fx["vol_prcnt"], fx["vol_margin"],
                                 device=device)
    assert torch.equal(bits(origin2), bits(origin)) and dim2 == dim


@pytest.mark.parametrize("name", ["general", "edge"])
def test_fixture_through_the_c_entry_point(device, golden_dir, name):
    from cnrma_amd.fusion import quantile_finish
    fx, proj, depth = fixture_views(golden_dir, name)
    q_lo, q_hi = 1 - fx["vol_prcnt"], fx["vol_prcnt"]
    values, counts = raw_bounds(device, torch.from_numpy(fx["pinv"]), depth, q_lo, q_hi, fx["max_depth"])
    assert counts.tolist() == fx["counts"].tolist() and same(values, fx["values"])
    for i, q in enumerate((q_lo, q_hi)):                                 # and the wrapper's finish of them is the recorded np.quantile
        got = quantile_finish(values[i, :, 0], values[i, :, 1], fx["n"], q, counts[1:])
        assert np.array_equal(got.view(np.uint32), fx["quantiles"][i].view(np.uint32))


# ---------------------------------------------------------------------------------------------------- few points
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("vol_prcnt", [0.5, 0.995, 1.0])
def test_one_two_and_three_points(device, n, vol_prcnt):
    """a single 1 x n map: with one point the clipped k + 1 is the point itself"""
    proj = torch.from_numpy(look_at((0.2, -1.0, 0.5), (0.0, 1.0, 0.4), 12.0, 1.5, 0.5)[0].astype(np.float32))[None]
    depth = torch.tensor([[[1.25, 0.75, 2.5][:n]]])
    pts = check_raw(device, proj, depth, vol_prcnt)
    assert len(pts) == n
    check_scene(device, proj, depth, vol_prcnt=vol_prcnt)


def test_no_usable_pixel_raises(device):
    from cnrma_amd.fusion import scene_bounds
    proj, _ = small_scene(2, 4, 6, seed=1)
    for depth in (torch.zeros(2, 4, 6), torch.full((2, 4, 6), math.nan), torch.full((2, 4, 6), 5.0)):
        with pytest.raises(ValueError, match="no pixel with a usable depth"):
            scene_bounds(proj, depth, 0.04, max_depth=3.0, device=device)
        assert len(check_raw(device, proj, depth, 0.995, max_depth=3.0)) == 0
    with pytest.raises(ValueError, match="no pixel with a usable depth"):
        scene_bounds(proj[:0], torch.zeros(0, 4, 6), 0.04, device=device)             # V = 0
    for shape in ((0, 4, 6), (2, 0, 6), (2, 4, 0)):
        values, counts = raw_bounds(device, inverses(proj[:shape[0]]), torch.zeros(shape), 0.005, 0.995)
        assert counts.tolist() == [0, 0, 0, 0] and bool((values == CANARY_F).all())


# ---------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 9), (1, 8, 8), (1, 5, 13), (1, 15, 17), (2, 8, 16), (1, 1, 257), (3, 85, 3),
                                   (3, 419, 421)])
def test_sizes_inside_canaried_buffers(device, shape):
    """V*H*W of 1, 63, 64, 65, 255, 256, 257; three views whose 255 pixels end inside a tile; 2070 tiles of 256 pixels: more than the
    2048 blocks of one grid sweep"""
    proj, depth = small_scene(*shape, seed=sum(shape))
    if shape == (1, 1, 1):
        depth = torch.full((1, 1, 1), 1.5)
    pts = check_raw(device, proj, depth, 0.995)
    assert len(pts) > 0
    check_scene(device, proj, depth)


def test_rejected_arguments(device):
    from cnrma_amd import _lib
    from cnrma_amd._lib import ptr, stream
    lib = _lib.load_prep()
    nbytes = lib.cnrma_prep_bounds_workspace_bytes()
    pinv, depth, values = (torch.zeros(64, device=device) for _ in range(3))
    depth += 1
    pinv[:16] = torch.eye(4).reshape(-1)
    ws, counts = torch.zeros(nbytes, dtype=torch.uint8, device=device), torch.zeros(4, dtype=torch.int64, device=device)

    def rc(V=1, H=2, W=2, q_lo=0.005, q_hi=0.995, size=nbytes, **kw):
        p = dict(pinv=ptr(pinv), depth=ptr(depth), ws=ptr(ws), values=ptr(values), counts=ptr(counts))
        p.update(kw)
        return lib.cnrma_prep_depth_bounds_f32(p["pinv"], p["depth"], V, H, W, math.inf, q_lo, q_hi, p["ws"], size, p["values"],
                                               p["counts"], stream())
    assert rc() == 0 and rc(V=0) == 0 and rc(H=0) == 0 and rc(q_lo=0.0, q_hi=1.0) == 0
    for bad in (dict(V=-1), dict(H=-1), dict(W=-1), dict(V=2048, H=1024, W=1024), dict(q_lo=-0.5), dict(q_hi=1.5),
                dict(q_hi=math.nan), dict(size=nbytes - 1), dict(ws=None), dict(ws=ptr(ws) + 1), dict(values=None), dict(counts=None),
                dict(pinv=None), dict(depth=None)):
        assert rc(**bad) == -22, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- quantiles and views
@pytest.mark.parametrize("vol_prcnt", [0.5, 1.0, 0.995])
def test_quantiles(device, golden_dir, vol_prcnt):
    """0.5: both quantiles are the median; 1.0: q_lo == 0, the minimum and the maximum; 0.995: the reference's default"""
    fx, proj, depth = fixture_views(golden_dir, "general")
    check_raw(device, proj, depth, vol_prcnt, max_depth=3.0)
    check_scene(device, proj, depth, max_depth=3.0, vol_prcnt=vol_prcnt, vol_margin=0.25)


def test_every_prefix_of_views(device, golden_dir):
    fx, proj, depth = fixture_views(golden_dir, "general")
    for k in range(1, len(proj) + 1):
        check_raw(device, proj[:k], depth[:k], 0.995, max_depth=3.0)
        check_scene(device, proj[:k], depth[:k], max_depth=3.0)


def test_view_order_does_not_matter(device, golden_dir):
    from cnrma_amd.fusion import scene_bounds
    fx, proj, depth = fixture_views(golden_dir, "general")
    want = check_scene(device, proj, depth, max_depth=3.0)
    for order in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        got = scene_bounds(proj[order], depth[order], 0.04, 3.0, device=device)
        assert torch.equal(bits(got[0]), bits(want[0])) and got[1] == want[1]
    pinv = torch.from_numpy(fx["pinv"])
    got = scene_bounds(proj[[2, 0, 1]], depth[[2, 0, 1]], 0.04, 3.0, device=device, pinv=pinv[[2, 0, 1]])
    assert torch.equal(bits(got[0]), bits(torch.from_numpy(fx["origin"]))) and got[1] == fx["voxel_dim"]


# ---------------------------------------------------------------------------------------------------- NaN and zeros
def test_nan_on_one_axis(device, golden_dir):
    """a Pinv with a NaN in row 1: x stays finite, so the pixels are kept; y holds NaNs, and its quantile is NaN as numpy's is"""
    from cnrma_amd.fusion import quantile_finish
    fx, proj, depth = fixture_views(golden_dir, "general")
    pinv = torch.from_numpy(fx["pinv"]).clone()
    pinv[1, 1, 2] = math.nan
    pts = check_raw(device, proj, depth, 0.995, max_depth=3.0, pinv=pinv)
    values, counts = raw_bounds(device, pinv, depth, 0.005, 0.995, 3.0)
    assert counts[0] == len(pts) and counts[1] == 0 and 0 < counts[2] < counts[0] and counts[3] == 0
    for i, q in enumerate((0.005, 0.995)):
        got = quantile_finish(values[i, :, 0], values[i, :, 1], int(counts[0]), q, counts[1:])
        exp = np.quantile(pts, q, axis=0)
        assert np.isnan(got[1]) and np.isnan(exp[1]) and not np.isnan(got[[0, 2]]).any()
        assert np.array_equal(got[[0, 2]].view(np.uint32), exp[[0, 2]].view(np.uint32))


def test_zeros_of_both_signs_at_the_rank(device):
    """x = -0.0 where the depth is positive, +0.0 where it is negative (row 0 of Pinv is all -0.0): every rank holds a zero of one sign
    or the other; y and z are ordinary"""
    pinv = torch.tensor([[[-0.0, -0.0, -0.0, -0.0], [1.0, 0.0, -3.0, 0.0], [0.0, 1.0, 0.0, 2.0], [0.0, 0.0, 1.0, 0.0]]])
    depth = torch.tensor([[[1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 0.5], [-0.5, 8.0, -8.0, 1.0, -1.0, 2.0, 0.0]]])
    pts = BO.cloud(None, depth, pinv=pinv)
    sign = np.signbit(pts[:, 0])
    assert len(pts) == 13 and (pts[:, 0] == 0).all() and sign.any() and not sign.all()
    for vol_prcnt in (0.5, 0.75, 1.0):
        values, counts = raw_bounds(device, pinv, depth, 1 - vol_prcnt, vol_prcnt)
        exp, _ = BO.order_statistics(pts, 1 - vol_prcnt, vol_prcnt)
        assert counts.tolist() == [13, 0, 0, 0] and same(values, exp) and bool((values[:, 0] == 0).all())


# ---------------------------------------------------------------------------------------------------- scale
def ring_views(V, H, W, seed):
    """V cameras on test_fusion_gpu's ring around a 4.8 x 4.8 x 2.4 m volume, depth 0.5 - 4.5 m, 5 % holes"""
    rng = np.random.default_rng(seed)
    ext = np.array([4.8, 4.8, 2.4])
    centre, size = 0.5 * ext, float(np.linalg.norm(ext))
    dist = 1.0 + size
    proj = np.stack([look_at(centre + [dist * np.cos(a), dist * np.sin(a), 0.3 * dist], centre, 0.8 * W * dist / size, W / 2, H / 2)[0]
                     for a in 2 * np.pi * (np.arange(V) * 0.37 + 0.1)]).astype(np.float32)
    depth = torch.from_numpy(rng.random((V, H, W), dtype=np.float32)) * 4.0 + 0.5
    depth[torch.from_numpy(rng.random((V, H, W), dtype=np.float32) < 0.05)] = 0
    return torch.from_numpy(proj), depth


def test_more_than_two_to_the_24_points(device):
    """60 views of 480 x 640 with 5 % holes: n = 17.5 M > 2^24, and not a float32 -- a count that passed through a float would differ.
    (56 views would hold 16.3 M kept pixels, fewer than 2^24 = 16.8 M.)"""
    from cnrma_amd.fusion import scene_bounds
    proj, depth = ring_views(60, 480, 640, seed=3)
    pinv = inverses(proj)
    pts = BO.cloud(proj, depth, pinv=pinv)
    n = len(pts)
    assert n > 2 ** 24 and int(np.float32(n)) != n
    exp_origin, exp_dim, exp_q = BO.bounds_of_cloud(pts, 0.04)
    depth = depth.to(device)
    values, counts = raw_bounds(device, pinv, depth, 1 - .995, .995)
    assert counts.tolist() == [n, 0, 0, 0]
    origin, dim = scene_bounds(proj, depth, 0.04, device=device)
    assert torch.equal(bits(origin), bits(exp_origin)) and dim == exp_dim
    exp_values, _ = BO.order_statistics(pts, 1 - .995, .995)
    assert same(values, exp_values)


# ---------------------------------------------------------------------------------------------------- end to end
def test_fuse_scene_on_the_sphere(device):
    from cnrma_amd.fusion import TSDFFusion, fuse_scene
    sc = sphere_scene()
    exp_origin, exp_dim, _ = BO.bounds(sc["proj"], sc["depth"], 0.04, 3.0, .995, 1.5)
    tsdf = fuse_scene(sc["proj"], sc["depth"], device=device, batch=4)              # two launches: 4 + 2 views
    assert torch.equal(bits(tsdf.origin.reshape(3)), bits(exp_origin)) and list(tsdf.tsdf_vol.shape) == exp_dim
    assert tsdf.voxel_size == 0.04 and tsdf.attribute_vols == {}
    by_hand = TSDFFusion(exp_dim, 0.04, exp_origin, trunc_ratio=3, device=device, color=False, label=False)
    by_hand.integrate(sc["proj"], sc["depth"], max_depth=3.0)
    want = by_hand.get_tsdf()
    assert torch.equal(bits(tsdf.tsdf_vol), bits(want.tsdf_vol)) and int((want.tsdf_vol.abs() < 1).sum()) > 1000
    # with colour, and against the fusion oracle fed the oracle's bounds
    color = torch.rand(6, 3, 96, 128) * 255
    coloured = fuse_scene(sc["proj"], sc["depth"], color, device=device)
    exp = FO.fuse(tuple(exp_dim), 0.04, tuple(exp_origin.tolist()), sc["proj"], sc["depth"], color, None, max_depth=3.0)
    t, c = FO.finish(exp)
    assert torch.equal(bits(coloured.tsdf_vol), bits(t.view(exp_dim))) and torch.equal(bits(coloured.tsdf_vol), bits(tsdf.tsdf_vol))
    assert torch.equal(bits(coloured.attribute_vols["color"]), bits(c.view([3] + exp_dim)))


def test_fuse_scene_takes_the_bounds_from_200_of_many_frames(device):
    """203 tiny frames: the bounds come from frames linspace(0, 202, 200).astype(int), the fusion from all of them"""
    from cnrma_amd.fusion import TSDFFusion, fuse_scene
    proj, depth = small_scene(203, 4, 6, seed=9)
    inds = np.linspace(0, 202, 200).astype(int)
    assert len(set(inds)) == 200
    exp_origin, exp_dim, _ = BO.bounds(proj[inds], depth[inds], 0.08, 3.0, .9, 0.5)
    all_origin, all_dim, _ = BO.bounds(proj, depth, 0.08, 3.0, .9, 0.5)
    assert not torch.equal(exp_origin, all_origin)                                  # the subset matters
    tsdf = fuse_scene(proj, depth, voxel_size=0.08, vol_prcnt=.9, vol_margin=0.5, batch=64, device=device)
    assert torch.equal(bits(tsdf.origin.reshape(3)), bits(exp_origin)) and list(tsdf.tsdf_vol.shape) == exp_dim
    by_hand = TSDFFusion(exp_dim, 0.08, exp_origin, device=device, color=False)
    by_hand.integrate(proj, depth, max_depth=3.0)
    assert torch.equal(bits(tsdf.tsdf_vol), bits(by_hand.get_tsdf().tsdf_vol))
