"""GPU parity tests (-m gpu) of the aggregation half: HIP kernels (through the C-ABI) vs the golden vectors generated
from the reference and vs the oracle on fresh seeded inputs.

Bars (north_star): integer / index outputs bit-exact; fp32 within 1e-4.  What we actually hold is stricter:
geometry (places, ray parameters, dense volume) is bit-exact; weights are bit-exact except for the <= 31 tail
elements per thread chunk where torch's CPU sigmoid falls back to libm (see DESIGN.md "numerics")."""
import numpy as np
import pytest
import torch

from helpers import QUIRK_SCENES, QUIRK_SINGLE_VIEW, SCENES, bits_equal, count_mismatch, load_golden, t

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _scene(g, device):
    from cnrma_amd import rma
    feats = rma.to_nhwc(t(g["features"], device))
    # the inverse projection is pinned as an INPUT: torch.inverse (LAPACK) is not bit-stable across host CPUs, so the
    # golden value (computed where the reference ran) is what makes voxel ids comparable bit-for-bit
    pinv = t(g["proj_inv"], device)
    return feats, pinv, t(g["tsdf"], device)


@pytest.mark.parametrize("name", SCENES)
def test_host_projection_inverse_close_to_golden(name):
    from cnrma_amd import rma
    g = load_golden(name)
    pinv = rma.projection_inverse(t(g["projection"]), g["stride"])
    np.testing.assert_allclose(pinv.numpy(), g["proj_inv"], rtol=1e-4, atol=1e-5)


def test_library_is_the_hip_build(device):
    from cnrma_amd import _lib
    assert _lib.load().cnrma_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("shape", [(3, 8, 30, 40), (2, 32, 17, 23), (1, 5, 9, 7), (2, 64, 33, 65)])
def test_nchw_to_nhwc(device, shape):
    from cnrma_amd import rma
    x = torch.randn(*shape, device=device)
    assert torch.equal(rma.to_nhwc(x), x.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("name", SCENES)
def test_dense_unprojection_bit_exact(device, name):
    from cnrma_amd import rma
    g = load_golden(name)
    feats = rma.to_nhwc(t(g["features"], device))
    vol, cnt = rma.backproject_accum(feats, t(g["projection"]), g["dims"], g["voxel_size"], g["origin"], g["stride"])
    assert (cnt.cpu().numpy() == g["dense_count"]).all()
    assert count_mismatch(vol, g["dense_volume"]) == 0
    px, py, valid = rma.backproject_index(rma.scale_projection(t(g["projection"][0]), g["stride"]),
                                          g["features"].shape[-2:], g["dims"], g["voxel_size"], g["origin"], device)
    assert (valid.cpu().numpy().astype(bool) == g["view0_valid"]).all()
    ok = (np.abs(g["view0_px"]) < 2 ** 31 - 1000) & (np.abs(g["view0_py"]) < 2 ** 31 - 1000)
    assert (px.cpu().numpy()[ok] == g["view0_px"][ok]).all() and (py.cpu().numpy()[ok] == g["view0_py"][ok]).all()


@pytest.mark.parametrize("name", SCENES)
def test_ray_params_bit_exact(device, name):
    from cnrma_amd import rma
    g = load_golden(name)
    H, W = g["features"].shape[-2:]
    o, d = rma.ray_params(t(g["proj_inv"], device), H, W)
    assert count_mismatch(o, g["ray_o"]) == 0
    assert count_mismatch(d, g["ray_d"]) == 0


@pytest.mark.parametrize("single_march", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_neus_rows_vs_golden(device, name, single_march):
    from cnrma_amd import rma
    g = load_golden(name)
    feats, pinv, tsdf = _scene(g, device)
    rows, per_view, samples = rma.rma_view_rows(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"],
                                                g["thr"], with_samples=True, single_march=single_march)
    assert list(per_view.cpu().numpy()) == list(g["neus_counts"])        # kept set: same size per view
    rows = rows.cpu().numpy()
    exp = g["neus_rows"]
    assert count_mismatch(rows[:, :3], exp[:, :3]) == 0                      # places bit-exact
    assert count_mismatch(rows[:, 4:], exp[:, 4:]) == 0                      # gathered features bit-exact
    np.testing.assert_allclose(rows[:, 3], exp[:, 3], rtol=1e-6, atol=0)     # weights (<= 1 ulp, libm tail)
    assert count_mismatch(rows[:, 3], exp[:, 3]) <= max(8, rows.shape[0] // 50)
    # (ray, step) of view 0 = the reference's kept set, in the reference's order
    n0 = int(g["neus_counts"][0])
    if n0:
        s = samples.cpu().numpy()[:n0]
        assert (s[:, 0] == g["v0_ray"]).all() and (s[:, 1] == g["v0_step"]).all()


@pytest.mark.parametrize("name", SCENES)
def test_aggregate_points_vs_golden(device, name):
    from cnrma_amd import rma
    g = load_golden(name)
    feats, pinv, tsdf = _scene(g, device)
    pts, info = rma.aggregate_rows(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"])
    exp = g["points"]
    assert info["M"] == exp.shape[0]
    pts = pts.cpu().numpy()
    assert count_mismatch(pts[:, :3], exp[:, :3]) == 0
    np.testing.assert_allclose(pts[:, 3:], exp[:, 3:], rtol=TOL, atol=TOL)
    np.testing.assert_allclose(pts[:, 3:], exp[:, 3:], rtol=2e-6, atol=1e-7)  # what we actually achieve


@pytest.mark.parametrize("name", SCENES)
def test_fused_select_matches_switch_pointcloud(device, name):
    from cnrma_amd import rma
    g = load_golden(name)
    feats, pinv, tsdf = _scene(g, device)
    M = g["points"].shape[0]
    mask = np.unpackbits(g["sel_mask"])[:M].astype(bool)
    c, f, info = rma.aggregate_points(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"],
                                      offset=g["sel_offset"], mask=mask)
    assert c.shape[0] == g["sel_coords"].shape[0]
    assert count_mismatch(c, g["sel_coords"]) == 0
    np.testing.assert_allclose(f.cpu().numpy(), g["sel_feats"], rtol=2e-6, atol=1e-7)
    # same thing through the numpy-global-RNG sampler (reference semantics of sample_points)
    np.random.seed(7)
    c2, f2, _ = rma.aggregate_points(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"],
                                     offset=g["sel_offset"], max_points=int(g["sel_max_points"]), sampler="numpy")
    assert torch.equal(c, c2) and torch.equal(f, f2)
    # and the stand-alone select kernel on the golden point matrix
    c3, f3 = rma.select_rows(t(g["points"], device), g["sel_offset"], mask)
    assert count_mismatch(c3, g["sel_coords"]) == 0 and count_mismatch(f3, g["sel_feats"]) == 0


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_depth_rows_vs_golden(device, name, k):
    from cnrma_amd import rma
    g = load_golden(name)
    feats, pinv, tsdf = _scene(g, device)
    rows, per_view = rma.rma_view_rows(feats[:1], pinv[:1], tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"],
                                       mode="depth", select_grids=k)
    exp = g[f"depth_rows_k{k}"]
    assert rows.shape[0] == exp.shape[0]
    if exp.shape[0]:
        assert count_mismatch(rows, exp) == 0


def test_device_sampler_keeps_exactly_max_points(device):
    from cnrma_amd import rma
    g = load_golden("tiny")
    feats, pinv, tsdf = _scene(g, device)
    c, f, info = rma.aggregate_points(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"],
                                      max_points=300, sampler="device")
    assert c.shape[0] == 300 and f.shape[0] == 300 and info["M"] == g["points"].shape[0]
    # rows are a subset of the full set, in order
    full, _ = rma.aggregate_rows(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"])
    key = {tuple(r) for r in full[:, :3].cpu().numpy().view(np.uint32)}
    assert all(tuple(r) in key for r in c.cpu().numpy().view(np.uint32))


def test_device_sampler_is_exact_uniform_and_deterministic(device):
    from cnrma_amd import rma
    M, keep = 1_000_003, 250_000
    m_dev = torch.tensor([M], dtype=torch.int32, device=device)
    a = rma.sample_mask_device(m_dev, M, keep, seed=123)
    b = rma.sample_mask_device(m_dev, M, keep, seed=123)
    c = rma.sample_mask_device(m_dev, M, keep, seed=124)
    assert int(a.sum()) == keep and torch.equal(a, b) and int(c.sum()) == keep and not torch.equal(a, c)
    # uniformity: every tenth of the index range holds ~keep/10 selected rows (binomial sd ~ 137)
    parts = a.view(-1)[: M // 10 * 10].view(10, -1).sum(dim=1).float()
    assert (parts - keep / 10).abs().max() < 900
    assert int(rma.sample_mask_device(m_dev, M, M + 5, seed=1).sum()) == M       # keep everything when M <= n_keep
    for k in (1, 2, 999_999):
        assert int(rma.sample_mask_device(m_dev, M, k, seed=7).sum()) == k


def test_all_views_empty_raises_like_reference(device):
    from cnrma_amd import rma
    g = load_golden("edge_empty_view")
    feats, pinv, tsdf = _scene(g, device)
    with pytest.raises(TypeError):
        rma.aggregate_rows(feats[:1], pinv[:1], tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"])


@pytest.mark.parametrize("seed,V", [(11, 3)])
def test_neus_vs_oracle_at_scannet_shape(device, seed, V):
    """Fresh seeded scene at the real per-view shape (120x160x32 -> 192x192x80, N=300): HIP vs oracle."""
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    sc = synth.make_scene("S", seed=seed, boxes=4, V=V)
    proj, feat, tsdf = sc["projection"][:, 0], sc["features"][:, 0], sc["tsdf"][0, 0]
    exp = O.aggregate_rma(proj, feat, tsdf, sc["dims"], 0.04, sc["origin"], sc["stride"], 300, 0.05, return_raw=True)[1]
    feats = rma.to_nhwc(feat.to(device))
    pinv = rma.projection_inverse(proj, sc["stride"]).to(device)
    rows, per_view = rma.rma_view_rows(feats, pinv, tsdf.to(device), sc["dims"], 0.04, sc["origin"], 300, 0.05)
    rows = rows.cpu().numpy()
    exp = exp.numpy()
    # exclude-and-count: the kept set may differ only by samples whose weight lies within 1e-6 of the threshold
    # (the <= 1-ulp libm tail of torch's CPU sigmoid); such rows are matched out by their bit-exact (place, feature) key,
    # counted, bounded -- and everything else is compared as strictly as when the sets are equal
    excluded = 0
    if rows.shape[0] != exp.shape[0] or count_mismatch(rows[:, :3], exp[:, :3]) != 0:
        def keys(a):
            k = np.ascontiguousarray(np.concatenate((a[:, :3], a[:, 4:6]), axis=1)).view(np.uint32)
            return [r.tobytes() for r in k]
        kg, ke = keys(rows), keys(exp)
        sg, se = set(kg), set(ke)
        only_g = np.array([k not in se for k in kg])
        only_e = np.array([k not in sg for k in ke])
        assert (np.abs(rows[only_g, 3] - 0.05) < 1e-6).all() and (np.abs(exp[only_e, 3] - 0.05) < 1e-6).all()
        excluded = int(only_g.sum() + only_e.sum())
        assert excluded <= max(4, exp.shape[0] // 100000), excluded
        rows, exp = rows[~only_g], exp[~only_e]
    assert rows.shape == exp.shape
    assert count_mismatch(rows[:, :3], exp[:, :3]) == 0
    assert count_mismatch(rows[:, 4:], exp[:, 4:]) == 0
    np.testing.assert_allclose(rows[:, 3], exp[:, 3], rtol=1e-6)
    assert count_mismatch(rows[:, 3], exp[:, 3]) < 1000
    print(f"threshold-adjacent samples excluded: {excluded} of {exp.shape[0]}")


def test_dense_vs_oracle_at_scannet_shape(device):
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    sc = synth.make_scene("S", seed=5, V=3)
    proj, feat = sc["projection"][:, 0], sc["features"][:, 0]
    vol, cnt = O.backproject_accum(sc["dims"], 0.04, sc["origin"], proj, feat, sc["stride"])
    v2, c2 = rma.backproject_accum(rma.to_nhwc(feat.to(device)), proj, sc["dims"], 0.04, sc["origin"], sc["stride"])
    assert torch.equal(c2.cpu().to(torch.int64), cnt)
    assert count_mismatch(v2, vol) == 0


def test_baseline_config0_plumbing_vs_oracle(device):
    """BASELINE.json configs[0]: 4 views, 64 ch, 128x128 maps (stride 1) -> 64^3 grid, the reference's CPU-runnable case:
    dense volume bit-exact, aggregated points (places bit-exact, features 1e-4), selection + voxelisation identical."""
    from cnrma_amd import rma, synth
    from cnrma_amd import sparse as S
    from oracle import rma_oracle as O
    sc = synth.make_scene("P", seed=0)
    proj, feat, tsdf = sc["projection"][:, 0], sc["features"][:, 0], sc["tsdf"][0, 0]
    vol, cnt = O.backproject_accum(sc["dims"], 0.04, sc["origin"], proj, feat, sc["stride"])
    pts = O.aggregate_rma(proj, feat, tsdf, sc["dims"], 0.04, sc["origin"], sc["stride"])
    nhwc = rma.to_nhwc(feat.to(device))
    v2, c2 = rma.backproject_accum(nhwc, proj, sc["dims"], 0.04, sc["origin"], sc["stride"])
    assert torch.equal(c2.cpu().long(), cnt) and count_mismatch(v2, vol) == 0
    pinv = rma.projection_inverse(proj, sc["stride"]).to(device)
    got, info = rma.aggregate_rows(nhwc, pinv, tsdf.to(device), sc["dims"], 0.04, sc["origin"])
    assert info["M"] == pts.shape[0]
    assert count_mismatch(got[:, :3], pts[:, :3]) == 0
    np.testing.assert_allclose(got[:, 3:].cpu().numpy(), pts[:, 3:].numpy(), rtol=TOL, atol=TOL)
    np.random.seed(11)
    mask = O.sample_mask_numpy(pts.shape[0], 100000)
    c, f, _ = rma.aggregate_points(nhwc, pinv, tsdf.to(device), sc["dims"], 0.04, sc["origin"], offset=(0.1, -0.2, 0.3), mask=mask)
    co, fo = O.select_rows(pts, (0.1, -0.2, 0.3), mask)
    assert count_mismatch(c, co) == 0
    st, src = S.voxelize(c, f, 0.01, row_order="first")
    Cq, Fq, first = O.voxelize(co, fo, 0.01)
    assert torch.equal(st.C.cpu(), Cq) and torch.equal(src.cpu().long(), first)


def test_scannet_test_grid_256_vs_oracle(device):
    """ray_marching_scannet.py test shape (grid 256x256x96): indexing at the largest configured grid, 2 views"""
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    sc = synth.make_scene("St", seed=2, boxes=3, V=2)
    proj, feat, tsdf = sc["projection"][:, 0], sc["features"][:, 0], sc["tsdf"][0, 0]
    vol, cnt = O.backproject_accum(sc["dims"], 0.04, sc["origin"], proj, feat, sc["stride"])
    raw = O.aggregate_rma(proj, feat, tsdf, sc["dims"], 0.04, sc["origin"], sc["stride"], return_raw=True)[1]
    nhwc = rma.to_nhwc(feat.to(device))
    v2, c2 = rma.backproject_accum(nhwc, proj, sc["dims"], 0.04, sc["origin"], sc["stride"])
    assert torch.equal(c2.cpu().long(), cnt) and count_mismatch(v2, vol) == 0
    pinv = rma.projection_inverse(proj, sc["stride"]).to(device)
    rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf.to(device), sc["dims"], 0.04, sc["origin"], 300, 0.05)
    assert rows.shape[0] == raw.shape[0]
    assert count_mismatch(rows[:, :3], raw[:, :3]) == 0 and count_mismatch(rows[:, 4:], raw[:, 4:]) == 0
    np.testing.assert_allclose(rows[:, 3].cpu().numpy(), raw[:, 3].numpy(), rtol=1e-6)


@pytest.mark.parametrize("max_points", [None, 700])
def test_aggregation_backward_vs_oracle_autograd(device, max_points):
    """gradient of the aggregated point features w.r.t. the 2D feature maps (first piece): the HIP
    backward (one lane group per ray over its kept-sample records) == torch autograd through the oracle"""
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    sc = synth.make_scene("tiny", seed=3)
    proj, tsdf = sc["projection"][:, 0], sc["tsdf"][0, 0]
    f_cpu = sc["features"][:, 0].clone().requires_grad_(True)
    pts = O.aggregate_rma(proj, f_cpu, tsdf, sc["dims"], 0.04, sc["origin"], sc["stride"])
    mask = None
    if max_points is not None:
        np.random.seed(5)
        mask = O.sample_mask_numpy(pts.shape[0], max_points)
    sel = pts[:, 3:] if mask is None else pts[torch.from_numpy(mask)][:, 3:]
    g = torch.randn(sel.shape, generator=torch.Generator().manual_seed(1))
    (sel * g).sum().backward()

    f_gpu = sc["features"][:, 0].clone().to(device).requires_grad_(True)
    pinv = rma.projection_inverse(proj, sc["stride"]).to(device)
    coords, feats = rma.AggregatePoints.apply(f_gpu, pinv, tsdf.to(device), sc["dims"], 0.04, sc["origin"], 300, 0.05,
                                              (0.0, 0.0, 0.0), max_points, "numpy", mask)
    assert not coords.requires_grad and feats.requires_grad and feats.shape == sel.shape
    np.testing.assert_allclose(feats.detach().cpu().numpy(), sel.detach().numpy(), rtol=1e-5, atol=1e-6)
    (feats * g.to(device)).sum().backward()
    np.testing.assert_allclose(f_gpu.grad.cpu().numpy(), f_cpu.grad.numpy(), rtol=1e-5, atol=1e-6)
    assert float(f_gpu.grad.abs().sum()) > 0


def test_dense_unprojection_backward_vs_oracle_autograd(device):
    """gradient of the mean feature volume w.r.t. the 2D feature maps: float-atomic scatter == torch autograd through the
    oracle's gather / mean (sum order differs: tolerance, not bits)"""
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    sc = synth.make_scene("tiny", seed=8)
    proj = sc["projection"][:, 0]
    f_cpu = sc["features"][:, 0].clone().requires_grad_(True)
    vol, cnt = O.backproject_accum(sc["dims"], 0.04, sc["origin"], proj, f_cpu, sc["stride"])
    g = torch.randn(vol.shape, generator=torch.Generator().manual_seed(3))
    (vol * g).sum().backward()
    f_gpu = sc["features"][:, 0].clone().to(device).requires_grad_(True)
    v2, c2 = rma.BackprojectAccum.apply(f_gpu, proj, sc["dims"], 0.04, sc["origin"], sc["stride"])
    assert count_mismatch(v2.detach(), vol.detach()) == 0 and torch.equal(c2.cpu(), cnt.to(torch.int32))
    (v2 * g.to(device)).sum().backward()
    ref = f_cpu.grad.numpy()
    np.testing.assert_allclose(f_gpu.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()))


@pytest.mark.parametrize("vs", [0.04, 0.01, 0.05, 0.0625, 0.037, 1.0 / 3.0])
def test_division_by_voxel_size_is_exact(device, vs):
    """the march divides by the voxel size with the correctly rounded reciprocal and two quotient refinements instead of
    the full IEEE expansion: the quotients must be bit-identical for every coordinate the march can produce"""
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr, stream
    g = torch.Generator(device=device).manual_seed(int(vs * 1e6))
    n = 1 << 25
    parts = [(torch.rand(n // 4, generator=g, device=device) - 0.3) * 30.0,            # coordinates of a room-sized grid
             (torch.rand(n // 4, generator=g, device=device) - 0.5) * 1e-3,            # around the origin
             torch.randn(n // 4, generator=g, device=device) * 1e3,                    # far outside
             (torch.randint(-4000, 4000, (n // 4,), generator=g, device=device).float() + 0.5) * vs]   # near rounding ties
    a = torch.cat(parts).contiguous()
    qf, qr = torch.empty_like(a), torch.empty_like(a)
    _lib.experiments(True)                 # the parity aid lives in libcnrma_hip_exp.so (same rma.hip, -DCNRMA_EXPERIMENTS)
    try:
        call("cnrma_debug_div_by_voxel_size_f32", ptr(a), a.numel(), float(vs), ptr(qf), ptr(qr), stream())
    finally:
        _lib.experiments(False)
    assert torch.equal(qf.view(torch.int32), qr.view(torch.int32))


def test_channels_last_features_need_no_layout_pass(device):
    """a feature tensor in torch.channels_last memory format is used in place (zero-copy view), same results"""
    from cnrma_amd import rma
    g = torch.Generator().manual_seed(3)
    f = torch.randn(3, 8, 12, 16, generator=g).to(device)
    a = rma.to_nhwc(f)
    fcl = f.contiguous(memory_format=torch.channels_last)
    b = rma.to_nhwc(fcl)
    assert b.data_ptr() == fcl.data_ptr() and b.is_contiguous() and torch.equal(a, b)


def test_dense_traversal_orders_give_identical_volumes(device):
    """every schedule of the dense kernel -- product default, the round-2 one-gather-at-a-time kernel, plain z-fastest
    order, two views in flight, LDS-transposed stores, the persistent lockstep grid over 32^3 bricks -- adds the same
    values in the same view order per voxel: volume and counts bit-identical (ScanNet-sized grid with ragged last
    bricks: Z = 80 is 2.5 bricks)"""
    from cnrma_amd import rma, synth
    sc = synth.make_scene((6, 32, 60, 80, (72, 100, 80), 4), seed=4)
    feat = rma.to_nhwc(sc["features"][:, 0].to(device))
    proj = sc["projection"][:, 0]
    try:
        rma.dense_tuning(variant=0, slab=0)
        vol0, cnt0 = rma.backproject_accum(feat, proj, sc["dims"], 0.04, (0.0, 0.0, 0.0), sc["stride"])
        assert int(cnt0.max()) > 0
        for kw in (dict(), dict(variant=0), dict(variant=1, slab=0), dict(variant=1, pipe=2), dict(variant=1, epi=1),
                   dict(variant=1, pipe=2, epi=1), dict(variant=1, st=32, lockstep=1),
                   dict(variant=1, st=32, lockstep=1, epi=1, pipe=2), dict(variant=1, st=16, zt=16, tt=4, zi=16),
                   dict(variant=2), dict(variant=2, slab=0), dict(variant=2, st=32, lockstep=1), dict(variant=2, st=32, lockstep=2),
                   dict(variant=2, st=24, lockstep=1), dict(variant=1, st=32, lockstep=1, lattice=1), dict(variant=1, st=32, lattice=1), dict(variant=1, own=1)):
            rma.dense_tuning(**kw)
            vol, cnt = rma.backproject_accum(feat, proj, sc["dims"], 0.04, (0.0, 0.0, 0.0), sc["stride"])
            assert torch.equal(vol, vol0) and torch.equal(cnt, cnt0), kw
    finally:
        rma.dense_tuning()


@pytest.mark.parametrize("name", SCENES)
def test_select_records_equals_mask_index_scatter(device, name):
    """the per-ray selection (no M-sized mask / index: cnrma_rma_select_records) emits exactly the rows of
    sample_mask_device + mask_to_index + the record scatter -- same subset, same order, same values"""
    from cnrma_amd import rma
    g = load_golden(name)
    feats, pinv, tsdf = _scene(g, device)
    m = rma._March(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], 300, g["thr"], "neus", 0)
    cnt, wsum, kept, overflow = m.march()
    off = rma.exclusive_scan(cnt)
    M = int(off[-1])
    m_dev = off[m.R:]
    one = torch.ones(1, dtype=torch.float32, device=device)
    assert M > 40
    for n_keep, cap_extra in ((M // 7, 100), (M + 5, 0), (1, 3), (M // 2, 0)):
        M_cap = M + cap_extra
        cap = min(M_cap, n_keep)
        mask = rma.sample_mask_device(m_dev, M_cap, n_keep, seed=321)
        sel, n_a = rma.mask_to_index(mask)
        ca = torch.zeros((cap, 3), device=device); fa = torch.zeros((cap, m.C), device=device); wa = torch.zeros((cap, 1), device=device)
        m.emit_rows(off, cap, kept, sel, one, (0.5, 0.25, 0.125), ca.data_ptr(), 3, wa.data_ptr(), 1, fa.data_ptr(), m.C, n_out_dev=n_a)
        rec, n_b = rma.select_records(off, kept, m_dev, M_cap, n_keep, cap, seed=321)
        cb = torch.zeros((cap, 3), device=device); fb = torch.zeros((cap, m.C), device=device); wb = torch.zeros((cap, 1), device=device)
        m.emit_records(rec, cap, n_b, one, (0.5, 0.25, 0.125), cb.data_ptr(), 3, wb.data_ptr(), 1, fb.data_ptr(), m.C)
        n = int(n_a)
        assert n == int(n_b) == min(M, n_keep)
        assert torch.equal(ca[:n], cb[:n]) and torch.equal(fa[:n], fb[:n]) and torch.equal(wa[:n], wb[:n])


@pytest.mark.parametrize("shape,seed", [("tiny", 0), ("S", 1), ("St", 2)])
def test_free_space_skipping_changes_nothing_in_the_march(device, shape, seed):
    """rma.MARCH_SKIP: rays jump over steps that are certain to land in voxels of the same table value (no-ops of the march,
    ray_marching.py:759-767) -- counts, fp64 weight sums and every kept-sample record (weight bits, step) equal those of the
    step-by-step march bit for bit, on furnished rooms at the plumbing, ScanNet-train and ScanNet-test shapes; the skip table
    itself is checked against its definition on the host"""
    import numpy as np
    from cnrma_amd import rma, synth
    V, C, H, W, dims, stride = synth.SHAPES[shape]
    sc = synth.make_scene((V, 8, H, W, dims, stride), seed=seed, boxes=3)
    feat = rma.to_nhwc(sc["features"][:, 0].to(device))
    pinv = rma.projection_inverse(sc["projection"][:, 0], stride).to(device)
    tsdf = sc["tsdf"][0, 0].to(device)
    m = rma._March(feat, pinv, tsdf, dims, 0.04, sc["origin"], 300, 0.05, "neus", 0)
    prev = rma.MARCH_SKIP
    try:
        rma.MARCH_SKIP = False
        c0, w0, k0, o0 = m.march()
        rma.MARCH_SKIP = True
        c1, w1, k1, o1 = m.march()
    finally:
        rma.MARCH_SKIP = prev
    assert int(o0[0]) == 0 and int(o1[0]) == 0
    assert torch.equal(c0, c1) and torch.equal(w0, w1) and int(c0.sum()) > 500
    live = torch.arange(k0.shape[1], device=device)[None, :] < c0[:, None]
    assert torch.equal(k0[live], k1[live])
    # ---- the table against its definition: radius R of a block = 4 x the largest r <= 4 with every block within Chebyshev
    # distance r inside the grid, uniform, and of the block's value
    X, Y, Z = dims
    bx, by, bz = -(-X // 4), -(-Y // 4), -(-Z // 4)
    radii = m._skip[:bx * by * bz].cpu().numpy().reshape(bx, by, bz)
    sig = torch.empty_like(tsdf)
    from cnrma_amd._lib import call, ptr
    from cnrma_amd.rma import stream
    call("cnrma_rma_sigmoid_table_f32", ptr(tsdf), tsdf.numel(), ptr(sig), stream())
    bits = sig.cpu().numpy().view(np.uint32).reshape(X, Y, Z)
    val = np.full((bx, by, bz), 0xFFFFFFFF, dtype=np.uint64)
    for i in range(X // 4):
        for j in range(Y // 4):
            blk = bits[4 * i:4 * i + 4, 4 * j:4 * j + 4, :Z // 4 * 4].reshape(4, 4, Z // 4, 4)
            same = (blk == blk[0:1, 0:1, :, 0:1]).all(axis=(0, 1, 3))
            val[i, j, :Z // 4] = np.where(same, blk[0, 0, :, 0].astype(np.uint64), 0xFFFFFFFF)
    rng = np.random.RandomState(seed)
    for _ in range(300):
        i, j, k = rng.randint(bx), rng.randint(by), rng.randint(bz)
        r = 0
        if val[i, j, k] != 0xFFFFFFFF:
            while r < 4:
                d = r + 1
                if min(i, j, k) - d < 0 or i + d >= bx or j + d >= by or k + d >= bz:
                    break
                if not (val[i - d:i + d + 1, j - d:j + d + 1, k - d:k + d + 1] == val[i, j, k]).all():
                    break
                r += 1
        assert radii[i, j, k] == 4 * r, (i, j, k, radii[i, j, k], r)
    assert (radii > 0).mean() > 0.05                                  # furnished rooms still have free space to skip


@pytest.mark.parametrize("n", [1, 63, 1023, 1024, 1025, 32767, 32768, 32769, 70001, 5_000_000])
def test_device_scans_match_torch_on_both_sides_of_the_single_launch_threshold(device, n):
    """cnrma_exclusive_scan_i32 / cnrma_mask_to_index: one block and one launch up to 32 768 items (round 6: the coarse levels'
    strided sets, the neck's unions), tile sums + apply above -- both against torch.cumsum, at the sizes around the switch"""
    from cnrma_amd import rma
    g = torch.Generator(device=device).manual_seed(n)
    cnt = torch.randint(0, 7, (n,), generator=g, device=device, dtype=torch.int32)
    off = rma.exclusive_scan(cnt)
    ref = torch.cat((torch.zeros(1, dtype=torch.int64, device=device), torch.cumsum(cnt.long(), 0)))
    assert off.shape[0] == n + 1 and torch.equal(off.long(), ref)
    mask = (torch.rand(n, generator=g, device=device) < 0.37).to(torch.uint8)
    sel, n_sel = rma.mask_to_index(mask)
    rank = torch.cumsum(mask.long(), 0) - mask.long()
    assert int(n_sel) == int(mask.sum())
    assert torch.equal(sel.long(), torch.where(mask.bool(), rank, torch.full_like(rank, -1)))


# ---------------------------------------------------------------------------------------------------------------------
# views that keep exactly one sample (ray_marching.py:781-782 / :930-931 inside the bare except of :277-287):
# cnrma_rma_drop_single_sample_views against a numpy model, then the eager aggregation against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------
_DROP_CASES = ("zero", "one_first", "one_last", "one_middle", "two_split", "two_one_ray", "large")


def _drop_view_counts(case, rpv, rng):
    c = np.zeros(rpv, dtype=np.int32)
    if case == "one_first":
        c[0] = 1
    elif case == "one_last":
        c[-1] = 1
    elif case == "one_middle":
        c[rpv // 2] = 1
    elif case == "two_split":
        if rpv == 1:
            c[0] = 2
        else:
            c[rpv // 3] = 1
            c[-1] = 1
    elif case == "two_one_ray":
        c[(rpv * 2) // 3] = 2
    elif case == "large":
        c[:] = rng.randint(0, 6, size=rpv)
        c[rpv // 2] += 7
    return c


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("V", [1, 3, 40])
@pytest.mark.parametrize("rpv", [1, 3, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 120 * 160, 480 * 640])
def test_drop_single_sample_views_kernel_vs_model(device, rpv, V, offset):
    """count / wsum of the views whose total is exactly 1 are zeroed, every other element -- and canaries on both sides of the
    range -- is bit-unchanged; the int4 path (rays_per_view % 4 == 0 on a 16-byte aligned base) and the scalar path
    (ragged rays_per_view, or a base one element off alignment); every per-view case at every view position"""
    from cnrma_amd._lib import call, ptr, stream
    rng = np.random.RandomState(rpv * 7 + V * 3 + offset)
    pre, post = 8 + offset, 8
    n = V * rpv
    for shift in range(len(_DROP_CASES) if V < len(_DROP_CASES) else 1):
        cases = [_DROP_CASES[(v + shift) % len(_DROP_CASES)] for v in range(V)]
        cnt = np.concatenate([_drop_view_counts(c, rpv, rng) for c in cases])
        wsum = rng.rand(n) * (cnt > 0)
        wsum[rng.rand(n) < 0.01] = 0.25                       # weight sums on rays without kept samples are left alone too
        cbuf = rng.randint(-3, 4, size=pre + n + post).astype(np.int32)      # canaries: anything, ones included
        wbuf = rng.rand(pre + n + post)
        cbuf[pre:pre + n], wbuf[pre:pre + n] = cnt, wsum
        cdev, wdev = t(cbuf, device), t(wbuf, device)
        base_c, base_w = cdev[pre:], wdev[pre:]
        assert (base_c.data_ptr() % 16 == 0) == (offset == 0)
        call("cnrma_rma_drop_single_sample_views", base_c.data_ptr(), base_w.data_ptr(), V, rpv, stream())
        exp_c, exp_w = cbuf.copy(), wbuf.copy()
        tot = cnt.reshape(V, rpv).sum(axis=1)
        for v in np.nonzero(tot == 1)[0]:
            exp_c[pre + v * rpv:pre + (v + 1) * rpv] = 0
            exp_w[pre + v * rpv:pre + (v + 1) * rpv] = 0.0
        got_c, got_w = cdev.cpu().numpy(), wdev.cpu().numpy()
        assert (got_c == exp_c).all(), (cases, np.nonzero(got_c != exp_c)[0][:8])
        assert (got_w.view(np.uint64) == exp_w.view(np.uint64)).all(), (cases, np.nonzero(got_w != exp_w)[0][:8])
        assert (tot == 1).any() == any(c.startswith("one") for c in cases)


def test_drop_single_sample_views_rejects_bad_arguments(device):
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr, stream
    c = torch.ones(8, dtype=torch.int32, device=device)
    w = torch.ones(8, dtype=torch.float64, device=device)
    for args in ((ptr(c), ptr(w), 0, 8), (ptr(c), ptr(w), -1, 8), (ptr(c), ptr(w), 1, 0), (ptr(c), ptr(w), 1, -4),
                 (None, ptr(w), 1, 8), (ptr(c), None, 1, 8)):
        with pytest.raises(_lib.CnrmaError, match="invalid argument"):
            call("cnrma_rma_drop_single_sample_views", *args, stream())
    torch.cuda.synchronize()
    assert int(c.sum()) == 8 and float(w.sum()) == 8.0


_QUIRK_MODES = [("neus", None), ("depth", 0), ("depth", 1), ("depth", 2)]


@pytest.mark.parametrize("name", QUIRK_SCENES)
@pytest.mark.parametrize("mode,k", _QUIRK_MODES)
def test_single_sample_view_drop_eager_vs_reference(device, name, mode, k):
    """rma_view_rows (no quirk) still returns the one row of a view the reference drops; the aggregation (quirk on) returns
    the reference's points and M, and exactly one row more per dropped view with reference_quirks=False"""
    from cnrma_amd import rma
    g = load_golden(name)
    tag = "neus" if mode == "neus" else f"depth_k{k}"
    feats, pinv, tsdf = _scene(g, device)
    kw = dict(mode=mode, select_grids=k or 0)
    rows, per_view = rma.rma_view_rows(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"], **kw)
    skipped = g[f"{tag}_skipped"]
    per_view = per_view.cpu().numpy()
    assert list(per_view) == [1 if s else int(c) for s, c in zip(skipped, g[f"{tag}_counts"])]
    rows = rows.cpu().numpy()
    start = np.concatenate(([0], np.cumsum(per_view)))
    single = np.concatenate([rows[start[v]:start[v + 1]] for v in range(len(skipped)) if skipped[v]] or [rows[:0]])
    kept = np.concatenate([rows[start[v]:start[v + 1]] for v in range(len(skipped)) if not skipped[v]] or [rows[:0]])
    for got, exp in ((single, g[f"{tag}_single_rows"]), (kept, g[f"{tag}_rows"])):
        assert got.shape == exp.shape
        assert count_mismatch(got[:, :3], exp[:, :3]) == 0 and count_mismatch(got[:, 4:], exp[:, 4:]) == 0
        np.testing.assert_allclose(got[:, 3], exp[:, 3], rtol=1e-6, atol=0)
    n_drop = int(skipped.sum())
    agg = (feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"])
    if g[f"{tag}_raises"]:
        with pytest.raises(TypeError):
            rma.aggregate_rows(*agg, **kw)
    else:
        exp = g[f"{tag}_points"]
        pts, info = rma.aggregate_rows(*agg, **kw)
        assert info["M"] == exp.shape[0]
        pts = pts.cpu().numpy()
        assert count_mismatch(pts[:, :3], exp[:, :3]) == 0
        np.testing.assert_allclose(pts[:, 3:], exp[:, 3:], rtol=2e-6, atol=1e-7)
    _, info = rma.aggregate_rows(*agg, reference_quirks=False, **kw)
    assert n_drop >= (1 if tag in ("neus", "depth_k0") else 0)
    assert info["M"] == g[f"{tag}_points"].shape[0] + n_drop


def test_single_view_of_one_sample_raises_like_reference(device):
    from cnrma_amd import rma
    g = load_golden(QUIRK_SINGLE_VIEW)
    feats, pinv, tsdf = _scene(g, device)
    agg = (feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"])
    with pytest.raises(TypeError):
        rma.aggregate_rows(*agg)
    _, info = rma.aggregate_rows(*agg, reference_quirks=False)
    assert info["M"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# the dense unprojection at the north-star size (40 views x 256 ch x 480x640 -> 192^3) against the oracle on a voxel sample
# ---------------------------------------------------------------------------------------------------------------------
def _dense_sample(dims, brick=(16, 16, 32), n_random=60000, seed=0):
    """linear voxel ids: the first, the last and one interior brick whole; both planes of every brick boundary along a
    cross of lines per axis; the 8 corners and a strip of each face; the rest uniformly random"""
    X, Y, Z = dims
    bx, by, bz = brick
    lin = lambda x, y, z: (np.asarray(x) * Y + np.asarray(y)) * Z + np.asarray(z)
    parts = []
    nb = (-(-X // bx), -(-Y // by), -(-Z // bz))
    for b in ((0, 0, 0), (nb[0] - 1, nb[1] - 1, nb[2] - 1), (nb[0] // 2 - 1, nb[1] // 2, nb[2] // 2)):
        x, y, z = np.meshgrid(np.arange(b[0] * bx, min(X, b[0] * bx + bx)), np.arange(b[1] * by, min(Y, b[1] * by + by)),
                              np.arange(b[2] * bz, min(Z, b[2] * bz + bz)), indexing="ij")
        parts.append(lin(x, y, z).ravel())
    ext, size = (X, Y, Z), (bx, by, bz)
    for a in range(3):
        planes = sorted({c for b in range(size[a], ext[a], size[a]) for c in (b - 1, b)})
        o1, o2 = [i for i in range(3) if i != a]
        for c in planes:
            for vary, fixed in ((o1, o2), (o2, o1)):
                coord = [None] * 3
                coord[a] = np.full(ext[vary], c)
                coord[vary] = np.arange(ext[vary])
                coord[fixed] = np.full(ext[vary], ext[fixed] // 2 + 3)
                parts.append(lin(*coord))
    corners = np.array([[x, y, z] for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)])
    parts.append(lin(corners[:, 0], corners[:, 1], corners[:, 2]))
    for a in range(3):
        o1, o2 = [i for i in range(3) if i != a]
        for c in (0, ext[a] - 1):
            u, w = np.meshgrid(np.arange(ext[o1]), np.arange(ext[o2] // 2 - 2, ext[o2] // 2 + 2), indexing="ij")
            coord = [None] * 3
            coord[a], coord[o1], coord[o2] = np.full(u.size, c), u.ravel(), w.ravel()
            parts.append(lin(*coord))
    rng = np.random.RandomState(seed)
    parts.append(rng.randint(0, X * Y * Z, size=n_random))
    return np.unique(np.concatenate(parts).astype(np.int64))


def test_dense_north_star_shape_vs_oracle_sample(device):
    """the dominant kernel at the shipped size -- default brick order over 12 x 12 x 6 bricks, 8 sweeps of 32 channels, 40
    views -- and its channels-last by-reference form (the plugin's hand-off) against the oracle on > 1e5 sampled voxels x 256
    channels: counts equal, volume bit-equal.  The oracle's pixel indices are computed on the host; the feature values it
    needs are gathered on the device by plain indexing (an exact copy), view by view.  Accumulating two views in the other
    order must break bit equality somewhere in the sample: the check sees the fp32 summation order"""
    import time
    from cnrma_amd import rma, synth
    from oracle import rma_oracle as O
    if torch.cuda.get_device_properties(0).total_memory < 64e9:
        pytest.skip("needs ~26 GB of device memory (peak measured on an MI355X)")
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats()
    sc = synth.make_scene("NS", seed=3, boxes=3, device=device)
    dims, stride, origin = sc["dims"], sc["stride"], sc["origin"]
    proj = sc["projection"][:, 0]
    nhwc = rma.to_nhwc(sc["features"][:, 0])
    del sc
    V, H, W, C = nhwc.shape
    assert (V, C, H, W, tuple(dims)) == (40, 256, 480, 640, (192, 192, 192))
    vol, cnt = rma.backproject_accum(nhwc, proj, dims, 0.04, origin, stride)
    feat_ref = torch.tensor([nhwc.data_ptr()], dtype=torch.int64, device=device)
    vol_r, cnt_r = rma.backproject_accum(None, proj, dims, 0.04, origin, stride, feat_ref=feat_ref, shape=(V, H, W, C))
    gidx = _dense_sample(dims)
    assert gidx.size >= 100_000
    gi = torch.from_numpy(gidx).to(device)
    got = [(v.view(C, -1)[:, gi].cpu(), c.view(-1)[gi].cpu().long()) for v, c in ((vol, cnt), (vol_r, cnt_r))]
    del vol, vol_r, cnt, cnt_r
    gathers = [(lambda f: (lambda py, px: f[py.to(device), px.to(device)].t().cpu()))(nhwc[v]) for v in range(V)]
    exp_v, exp_c = O.backproject_accum_voxels(dims, 0.04, origin, proj, gathers, stride, torch.from_numpy(gidx), hw=(H, W))
    for path, (gv, gc) in zip(("nhwc", "by reference"), got):
        assert torch.equal(gc, exp_c), path
        assert count_mismatch(gv, exp_v) == 0, path
    hist = np.bincount(exp_c.numpy(), minlength=V + 1)
    print(f"\nNS dense: {gidx.size} sampled voxels x {C} channels; views per voxel histogram {hist.tolist()}")
    assert hist[0] > 0 and hist[V // 2:].sum() > 0
    # negative control: the last two views swapped on the oracle side (a 20 000-voxel part of the sample)
    part = torch.from_numpy(gidx[::max(1, gidx.size // 20000)])
    sel = torch.from_numpy(np.searchsorted(gidx, part.numpy()))
    sw_v, sw_c = O.backproject_accum_voxels(dims, 0.04, origin, proj, gathers, stride, part, hw=(H, W),
                                            order=list(range(V - 2)) + [V - 1, V - 2])
    assert torch.equal(sw_c, exp_c[sel])
    assert count_mismatch(got[0][0][:, sel], sw_v) > 0
    print(f"NS dense: peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB, {time.time() - t0:.1f} s")
    del nhwc, gathers, feat_ref
    torch.cuda.empty_cache()
