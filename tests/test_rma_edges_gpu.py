"""GPU tests (-m gpu) of the aggregation kernels at edge geometry and on every channel path, against the oracle.

The golden tests run every fixture through the default launch choices.  Here the same kernels are driven through the
branches those choices never take at fixture sizes: free-space skipping forced on and off (it turns itself on from 4 M rays
only), the per-step sigmoid march, every channel path of the dense unprojection, of the row / feature emission and of both
backward kernels, and the fused layout + march launch on both sides of its fallback.  The edge geometry is that of the
edge_outside_axis fixture: a 50 x 45 x 27 grid (no side divisible by 4), cameras outside the grid, on a lattice plane and
above a corner, rays with exactly-zero direction components.
Bars: volumes, counts, places and features bit-exact; NeuS weights within 1 ulp (the libm tail of the CPU sigmoid, see
test_rma_gpu.py); gradients within the tolerance their float atomics / summation order allow."""
import numpy as np
import pytest
import torch

from helpers import SCENES, count_mismatch, load_golden, t
from oracle import rma_oracle as O

pytestmark = pytest.mark.gpu

EDGE = "edge_outside_axis"


def _rows_match(rows, exp, per_view, exp_counts):
    """rows [M, 4+C] of rma_view_rows against the oracle's / the reference's: per-view counts exact, places and features
    bit-exact, weights within 1 ulp"""
    rows = rows.cpu().numpy() if torch.is_tensor(rows) else rows
    assert list(per_view) == list(exp_counts)
    assert rows.shape == exp.shape
    assert count_mismatch(rows[:, :3], exp[:, :3]) == 0
    assert count_mismatch(rows[:, 4:], exp[:, 4:]) == 0
    np.testing.assert_allclose(rows[:, 3], exp[:, 3], rtol=1e-6, atol=0)
    assert count_mismatch(rows[:, 3], exp[:, 3]) <= max(8, rows.shape[0] // 50)


def _march_settings(table, skip):
    from cnrma_amd import rma
    prev = (rma.SIGMOID_TABLE, rma.MARCH_SKIP)
    rma.SIGMOID_TABLE, rma.MARCH_SKIP = table, skip
    return prev


def _restore(prev):
    from cnrma_amd import rma
    rma.SIGMOID_TABLE, rma.MARCH_SKIP = prev


def _oracle_neus(g, feats, tsdf, thr=None):
    """oracle rows of every view (ray parameters pinned through the fixture's proj_inv) and the per-view counts"""
    H, W = feats.shape[-2:]
    rows, counts = [], []
    for v in range(feats.shape[0]):
        ps = O.scale_projection(t(g["projection"][v]), g["stride"])
        r = O.rma_neus_view(ps, feats[v], tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"],
                            g["thr"] if thr is None else thr, o_d=O.ray_params(ps, H, W, t(g["proj_inv"][v])),
                            reference_quirks=False)                    # rma_view_rows keeps a one-sample view
        counts.append(0 if r is None else r.shape[0])
        if r is not None:
            rows.append(r)
    return (torch.cat(rows) if rows else torch.zeros(0, 4 + feats.shape[1])).numpy(), counts


# ---------------------------------------------------------------------------------------------------------------------
# the march of every golden scene, with free-space skipping forced on / off and with the per-step sigmoid kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table,skip", [(True, True), (True, False), (False, False)], ids=["skip", "noskip", "sigmoid"])
@pytest.mark.parametrize("name", SCENES)
def test_golden_neus_rows_in_every_march_configuration(device, name, table, skip):
    from cnrma_amd import rma
    g = load_golden(name)
    feats = rma.to_nhwc(t(g["features"], device))
    prev = _march_settings(table, skip)
    try:
        m = rma._March(feats, t(g["proj_inv"], device), t(g["tsdf"], device), g["dims"], g["voxel_size"], g["origin"],
                       g["n_steps"], g["thr"], "neus", 0)
        assert m.kept_cap() > 0
        cnt, wsum, kept, overflow = m.march()
        assert int(overflow[0]) == 0
        assert (getattr(m, "_skip", None) is not None) == skip
        rows, per_view = rma.rma_view_rows(feats, t(g["proj_inv"], device), t(g["tsdf"], device), g["dims"], g["voxel_size"],
                                           g["origin"], g["n_steps"], g["thr"], single_march=True)
    finally:
        _restore(prev)
    assert torch.equal(cnt.view(feats.shape[0], -1).sum(dim=1).cpu(), per_view.cpu())
    _rows_match(rows, g["neus_rows"], per_view.cpu().numpy(), g["neus_counts"])


# ---------------------------------------------------------------------------------------------------------------------
# free-space skipping at the edges of its own argument
# ---------------------------------------------------------------------------------------------------------------------
def _host_skip_table(bits, dims):
    """the skip table by its definition (csrc/rma.hip skip_blockval_kernel / skip_radius_kernel): a 4^3 block's value is the
    table value all its voxels share (none when they differ or the block sticks out of the grid); its radius is 4 r for the
    largest r <= 4 such that every block within Chebyshev distance r exists and holds that value"""
    X, Y, Z = dims
    bx, by, bz = -(-X // 4), -(-Y // 4), -(-Z // 4)
    NONE = np.uint64(1 << 40)
    val = np.full((bx, by, bz), NONE, dtype=np.uint64)
    fx, fy, fz = X // 4, Y // 4, Z // 4
    blk = bits[:4 * fx, :4 * fy, :4 * fz].reshape(fx, 4, fy, 4, fz, 4).astype(np.uint64)
    first = blk[:, 0:1, :, 0:1, :, 0:1]
    same = (blk == first).all(axis=(1, 3, 5))
    val[:fx, :fy, :fz] = np.where(same, first[:, 0, :, 0, :, 0], NONE)
    radius = np.zeros((bx, by, bz), dtype=np.int64)
    ok = val != NONE
    for r in range(1, 5):
        okr = np.zeros_like(ok)
        inner = (slice(r, bx - r), slice(r, by - r), slice(r, bz - r))
        if min(bx, by, bz) > 2 * r:
            c = val[inner]
            good = c != NONE
            for i in range(-r, r + 1):
                for j in range(-r, r + 1):
                    for k in range(-r, r + 1):
                        good &= val[r + i:bx - r + i, r + j:by - r + j, r + k:bz - r + k] == c
            okr[inner] = good
        ok = ok & okr
        radius += ok
    return val, 4 * radius


SKIP_DIMS = (62, 55, 45)       # every axis ends in a partial 4^3 block, and blocks of every radius (4 .. 16) exist


def _skip_variants():
    """TSDF variants on the cameras, origin and maps of edge_outside_axis, with the grid grown to SKIP_DIMS so that every
    skip radius occurs: uniform free space with single-voxel specks on the axial ray of view 0 and off it, and one-voxel
    walls across each axis at Chebyshev distance 4r - 1, 4r and 4r + 1 from the border of block 0, r = 1..4 (the jump bound
    sits exactly at such distances)"""
    g = dict(load_golden(EDGE))
    g["dims"] = SKIP_DIMS
    X, Y, Z = g["dims"]
    out = []
    free = np.full((X, Y, Z), -1.0, np.float32)
    specks = free.copy()
    for x in (16, 28, 40):              # voxels (x, 21, 14) lie on the axial ray of view 0; x % 4 == 0: one voxel beyond the
        specks[x, 21, 14] = 1.0         # reach of a jump from two blocks back
    specks[20, 8, 20] = specks[44, 38, 4] = specks[5, 40, 22] = specks[30, 30, 13] = 0.5
    out.append(("specks", specks))
    for axis in range(3):
        for r in range(1, 5):
            for dd in (-1, 0, 1):
                w = 3 + 4 * r + dd                               # voxel distance 4r + dd from block 0's last layer (3)
                if w >= g["dims"][axis]:
                    continue
                v = free.copy()
                sl = [slice(None)] * 3
                sl[axis] = w
                v[tuple(sl)] = 1.0
                out.append((f"wall{axis}_{w}", v))
    return g, out


def test_free_space_skipping_at_block_and_radius_edges(device):
    """skip on / off give identical counts, fp64 weight sums and kept records on TSDFs built around the skip table's own
    edges, both equal the oracle, and the whole table (partial blocks included: radius 0, and they cap their neighbours)
    equals its host definition"""
    from cnrma_amd import rma
    from cnrma_amd._lib import call, ptr
    from cnrma_amd.rma import stream
    g, variants = _skip_variants()
    feats_cpu = t(g["features"])
    feats = rma.to_nhwc(feats_cpu.to(device))
    pinv = t(g["proj_inv"], device)
    X, Y, Z = g["dims"]
    assert X % 4 and Y % 4 and Z % 4
    jumps_possible, radii_seen = 0, set()
    for tag, tsdf_np in variants:
        tsdf_cpu = torch.from_numpy(tsdf_np)
        tsdf = tsdf_cpu.to(device)
        m = rma._March(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"], "neus", 0)
        prev = _march_settings(True, False)
        try:
            c0, w0, k0, o0 = m.march()
            rma.MARCH_SKIP = True
            c1, w1, k1, o1 = m.march()
        finally:
            _restore(prev)
        assert int(o0[0]) == 0 and int(o1[0]) == 0, tag
        assert torch.equal(c0, c1) and torch.equal(w0, w1), tag
        live = torch.arange(k0.shape[1], device=device)[None, :] < c0[:, None]
        assert torch.equal(k0[live], k1[live]), tag
        # against the oracle (rows through the emission of the skip march)
        prev = _march_settings(True, True)
        try:
            rows, per_view = rma.rma_view_rows(feats, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"],
                                               g["thr"], single_march=True)
        finally:
            _restore(prev)
        exp, counts = _oracle_neus(g, feats_cpu, tsdf_cpu)
        assert sum(counts) > 0, tag
        _rows_match(rows, exp, per_view.cpu().numpy(), counts)
        # the whole table against its definition
        sig = torch.empty_like(tsdf)
        call("cnrma_rma_sigmoid_table_f32", ptr(tsdf), tsdf.numel(), ptr(sig), stream())
        bits = sig.cpu().numpy().view(np.uint32).reshape(X, Y, Z)
        val, radius = _host_skip_table(bits, g["dims"])
        nb = val.size
        got = m._skip[:nb].cpu().numpy().reshape(val.shape).astype(np.int64)
        assert (got == radius).all(), (tag, np.argwhere(got != radius)[:5])
        assert (radius[-1] == 0).all() and (radius[:, -1] == 0).all() and (radius[:, :, -1] == 0).all()   # partial blocks
        jumps_possible += int((radius >= 8).sum())
        radii_seen |= set(np.unique(radius).tolist())
    assert jumps_possible > 0 and radii_seen == {0, 4, 8, 12, 16}


# ---------------------------------------------------------------------------------------------------------------------
# dense unprojection: every branch of backproject_accum_any
# ---------------------------------------------------------------------------------------------------------------------
DENSE_DIMS = [(1, 1, 1), (1, 7, 3), (17, 16, 33), (50, 45, 27)]


# 3, 5: plain kernel (C odd); 4, 12: LPV = 1; 8, 24: LPV = 2; 16, 48: LPV = 4; 32, 96: LPV = 8 (96: three channel sweeps)
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("C", [3, 5, 4, 12, 8, 24, 16, 48, 32, 96])
def test_dense_unprojection_every_channel_path(device, C, stride):
    from cnrma_amd import rma
    g = load_golden(EDGE)
    proj = t(g["projection"])
    H, W = (60, 80) if stride == 1 else (30, 40)
    f = torch.round(torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(C * 10 + stride)) * 64) / 64
    nhwc = rma.to_nhwc(f.to(device))
    seen = 0
    for dims in DENSE_DIMS:
        vol, cnt = rma.backproject_accum(nhwc, proj, dims, g["voxel_size"], g["origin"], stride)
        ev, ec = O.backproject_accum(dims, g["voxel_size"], g["origin"], proj, f, stride)
        assert torch.equal(cnt.cpu().long(), ec), (dims, C, stride)
        assert count_mismatch(vol, ev) == 0, (dims, C, stride)
        seen += int((ec > 0).sum())
    assert seen > 1000


def test_dense_unprojection_by_reference_at_48_channels(device):
    """cnrma_backproject_accum_ref_f32 (the maps' address in a device word, the static path's hand-off) on the LPV = 4 path"""
    from cnrma_amd import rma
    g = load_golden(EDGE)
    proj = t(g["projection"])
    f = torch.round(torch.randn(3, 48, 30, 40, generator=torch.Generator().manual_seed(48)) * 64) / 64
    nhwc = rma.to_nhwc(f.to(device))
    ref = torch.tensor([nhwc.data_ptr()], dtype=torch.int64, device=device)
    vol, cnt = rma.backproject_accum(None, proj, g["dims"], g["voxel_size"], g["origin"], 4, feat_ref=ref, shape=tuple(nhwc.shape))
    ev, ec = O.backproject_accum(g["dims"], g["voxel_size"], g["origin"], proj, f, 4)
    assert torch.equal(cnt.cpu().long(), ec) and count_mismatch(vol, ev) == 0
    v2, c2 = rma.backproject_accum(nhwc, proj, g["dims"], g["voxel_size"], g["origin"], 4)
    assert torch.equal(vol, v2) and torch.equal(cnt, c2)


# ---------------------------------------------------------------------------------------------------------------------
# emission: every channel path of the row emission and of the feature emission
# ---------------------------------------------------------------------------------------------------------------------
# 3, 5: LPR = 2 scalar (row stride 4 + C not a multiple of 4 either); 12: LPR = 2 vector; 40: LPR = 8 with a tail;
# 96: LPR = 8; 256: LPR = 64
@pytest.mark.parametrize("C", [3, 5, 12, 40, 96, 256])
def test_emission_every_channel_path(device, C):
    from cnrma_amd import rma
    g = load_golden(EDGE)
    f = torch.round(torch.randn(3, C, 30, 40, generator=torch.Generator().manual_seed(C)) * 64) / 64
    nhwc = rma.to_nhwc(f.to(device))
    pinv = t(g["proj_inv"], device)
    tsdf_cpu = t(g["tsdf"])
    tsdf = tsdf_cpu.to(device)
    rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"])
    exp, counts = _oracle_neus(g, f, tsdf_cpu)
    _rows_match(rows, exp, per_view.cpu().numpy(), counts)
    assert list(counts) == list(g["neus_counts"])                    # same geometry as the fixture: same kept set
    # scene aggregate (feature * w / mean(w)) through the row emission ...
    pts, info = rma.aggregate_rows(nhwc, pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"])
    ep = O.aggregate_rma(t(g["projection"]), f, tsdf_cpu, g["dims"], g["voxel_size"], g["origin"], g["stride"], g["n_steps"],
                         g["thr"], proj_inv=t(g["proj_inv"])).numpy()
    pts = pts.cpu().numpy()
    assert pts.shape == ep.shape
    assert count_mismatch(pts[:, :3], ep[:, :3]) == 0
    np.testing.assert_allclose(pts[:, 3:], ep[:, 3:], rtol=2e-6, atol=1e-7)
    # ... and through the feature emission of the static path (cnrma_rma_emit_features_f32): records of every row
    M = info["M"]
    rec, n_sel = rma.select_records(info["row_offset"], info["kept"], info["row_offset"][-1:], M, M, M, seed=5)
    assert int(n_sel) == M
    fe = rma.emit_point_features(info, rec, M, n_sel).cpu().numpy()
    assert count_mismatch(fe, pts[:, 3:]) == 0                      # records in row order: the same rows, bit for bit
    # and a sub-selection (records in selection order) against the same rows
    rec2, n2 = rma.select_records(info["row_offset"], info["kept"], info["row_offset"][-1:], M, M // 3, M // 3, seed=9)
    n2 = int(n2)
    fe2 = rma.emit_point_features(info, rec2, n2, None).cpu().numpy()
    r2 = rec2[:n2].cpu().numpy()
    off = info["row_offset"].cpu().numpy()
    kept = info["kept"].cpu().numpy()
    # row index of record (ray, step): its position among the ray's kept samples
    idx = np.array([off[r] + int(np.nonzero(kept[r, :off[r + 1] - off[r], 1] == s)[0][0]) for r, s in r2[:, :2]])
    assert count_mismatch(fe2, pts[idx, 3:]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# fused layout + march launch and its two-launch fallback
# ---------------------------------------------------------------------------------------------------------------------
def _fused_launch(V, C, H, W):
    """mirror of launch_march's choice (csrc/rma.hip): one fused launch when HW % 4 == C % 4 == 0 (16-byte accesses) and the
    layout half is at least 8x the march half"""
    n_layout = -(-H * W // 64) * -(-C // 64) * V
    n_march = V * -(-W // 16) * -(-H // 16)
    return (H * W) % 4 == 0 and C % 4 == 0 and n_layout >= 8 * n_march


FUSE_CASES = [(30, 40, 8), (29, 37, 8), (30, 40, 12), (30, 40, 6), (30, 40, 256), (30, 40, 136)]


def test_fuse_cases_cover_both_launch_forms():
    assert {_fused_launch(3, C, H, W) for H, W, C in FUSE_CASES} == {True, False}
    assert not _fused_launch(3, 8, 29, 37) and not _fused_launch(3, 6, 30, 40)


@pytest.mark.parametrize("H,W,C", FUSE_CASES)
def test_fused_layout_march_equals_two_launches(device, H, W, C):
    """m.march(layout_from=nchw) == to_nhwc + m.march(): the channels-last maps and every march output, bit for bit (the
    fused kernel at C = 256 / 136 -- 136: a partial 64-channel block --, the two-launch fallback when H*W % 4, C % 4 or the
    size ratio rule it out)"""
    from cnrma_amd import rma
    g = load_golden(EDGE)
    H0, W0 = g["features"].shape[-2:]
    # the fixture's cameras, re-scaled to an H x W map (pixel units scale with the map)
    proj = t(g["projection"]).clone()
    proj[:, 0] *= W / W0
    proj[:, 1] *= H / H0
    pinv = rma.projection_inverse(proj, g["stride"]).to(device)
    tsdf = t(g["tsdf"], device)
    f = torch.randn(3, C, H, W, generator=torch.Generator().manual_seed(H * W + C)).to(device)
    a = rma._March(torch.empty((3, H, W, C), device=device), pinv, tsdf, g["dims"], g["voxel_size"], g["origin"],
                   g["n_steps"], g["thr"], "neus", 0)
    a.feat.fill_(float("nan"))
    ca, wa, ka, oa = a.march(layout_from=f)
    b = rma._March(rma.to_nhwc(f), pinv, tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"], "neus", 0)
    cb, wb, kb, ob = b.march()
    assert torch.equal(a.feat, b.feat) and torch.equal(a.feat, f.permute(0, 2, 3, 1))
    assert int(oa[0]) == 0 and int(ob[0]) == 0
    assert torch.equal(ca, cb) and torch.equal(wa, wb) and int(ca.sum()) > 100
    live = torch.arange(ka.shape[1], device=device)[None, :] < ca[:, None]
    assert torch.equal(ka[live], kb[live])


# ---------------------------------------------------------------------------------------------------------------------
# backward kernels at training widths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8, 32, 40, 96])
def test_dense_backward_every_channel_path(device, C):
    """rma.BackprojectAccum's gradient (float atomics; LPV = 1 below 32 channels, LPV = 8 from 32 on, 40: a partial group)
    against autograd through the oracle with the maps in float64 (the projection stays fp32: same validity, same pixels)"""
    from cnrma_amd import rma
    g = load_golden(EDGE)
    proj = t(g["projection"])
    f = torch.randn(3, C, 30, 40, generator=torch.Generator().manual_seed(100 + C))
    f64 = f.double().requires_grad_(True)
    vol, cnt = O.backproject_accum(g["dims"], g["voxel_size"], g["origin"], proj, f64, g["stride"])
    gv = torch.randn(vol.shape, generator=torch.Generator().manual_seed(200 + C), dtype=torch.float64)
    (vol * gv).sum().backward()
    ref = f64.grad.numpy()
    fg = f.to(device).requires_grad_(True)
    v2, c2 = rma.BackprojectAccum.apply(fg, proj, g["dims"], g["voxel_size"], g["origin"], g["stride"])
    assert torch.equal(c2.cpu().long(), cnt)
    (v2 * gv.float().to(device)).sum().backward()
    got = fg.grad.cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    assert scale > 0
    assert float(np.abs(got - ref).max()) <= 1e-5 * scale
    assert (got[ref == 0] == 0).all()                                # pixels no voxel sees get nothing


@pytest.mark.parametrize("max_points", [None, 1500])
@pytest.mark.parametrize("C", [3, 8, 32, 40])
def test_aggregation_backward_every_channel_path(device, C, max_points):
    """rma.AggregatePoints's gradient (LPR = 1, 8, 32; 40: 32 lanes and a tail of 8 channels) against autograd through the
    oracle, with and without a sub-selection; exactly zero on every pixel whose ray kept nothing"""
    from cnrma_amd import rma
    g = load_golden(EDGE)
    proj, tsdf = t(g["projection"]), t(g["tsdf"])
    pinv_cpu = t(g["proj_inv"])
    f_cpu = torch.randn(3, C, 30, 40, generator=torch.Generator().manual_seed(300 + C)).requires_grad_(True)
    pts = O.aggregate_rma(proj, f_cpu, tsdf, g["dims"], g["voxel_size"], g["origin"], g["stride"], g["n_steps"], g["thr"],
                          proj_inv=pinv_cpu)
    mask = None
    if max_points is not None:
        assert max_points < pts.shape[0]
        np.random.seed(C)
        mask = O.sample_mask_numpy(pts.shape[0], max_points)
    sel = pts[:, 3:] if mask is None else pts[torch.from_numpy(mask)][:, 3:]
    gr = torch.randn(sel.shape, generator=torch.Generator().manual_seed(400 + C))
    (sel * gr).sum().backward()
    f_gpu = f_cpu.detach().clone().to(device).requires_grad_(True)
    coords, feats = rma.AggregatePoints.apply(f_gpu, pinv_cpu.to(device), tsdf.to(device), g["dims"], g["voxel_size"],
                                              g["origin"], g["n_steps"], g["thr"], (0.0, 0.0, 0.0), max_points, "numpy", mask)
    assert feats.shape == sel.shape
    np.testing.assert_allclose(feats.detach().cpu().numpy(), sel.detach().numpy(), rtol=1e-5, atol=1e-6)
    (feats * gr.to(device)).sum().backward()
    got, ref = f_gpu.grad.cpu().numpy(), f_cpu.grad.numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    assert float(np.abs(got).sum()) > 0
    # pixels whose ray kept nothing (from the oracle's kept set) get exactly zero, as do the ones no selected row reads
    H, W = 30, 40
    kept_any = np.zeros((3, H * W), dtype=bool)
    for v in range(3):
        ps = O.scale_projection(proj[v], g["stride"])
        _, dbg = O.rma_neus_view(ps, f_cpu[v].detach(), tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], g["thr"],
                                 o_d=O.ray_params(ps, H, W, pinv_cpu[v]), return_debug=True)
        if dbg is not None:
            kept_any[v, dbg["ray"].numpy()] = True
    none = ~kept_any.reshape(3, H, W)
    assert none.any() and (got.transpose(0, 2, 3, 1)[none] == 0).all()
    assert (got[ref == 0] == 0).all()
