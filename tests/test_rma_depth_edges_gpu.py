"""GPU tests (-m gpu) of the depth-mode ray march (csrc/rma.hip depth_count_kernel / depth_emit_kernel; reference
ray_projection_depth, ray_marching.py:809-956) at its edges, for select_grids = 0..4 and every channel path.

The fixture rma_depth_edges.npz (make_golden.py run_depth_edges: the reference's own rows, oracle == reference asserted
there and in test_rma_depth_edges_cpu.py) puts first sign changes at step 0 and at N-2 / N-3, so that the slot mask
`sel < 0 || sel >= N` works at both ends; its rays enter the grid straight into tsdf <= 0 (the change sits at the step before
the clipped interval's first in-grid sample), run along the axes, miss the grid in one view, and cross voxels of exactly 0.0,
-0.0, 1.0 and NaN.  Everything else here re-uses that geometry with other maps, map sizes and march lengths, against the
oracle (ray parameters pinned through proj_inv).
Bars: counts, places, weights and gathered features bit for bit (weights are j/k, nothing is rounded); aggregated features
f * w / mean(w) at rtol 2e-6 / atol 1e-7 (test_rma_gpu.py test_aggregate_points_vs_golden); gradients at rtol 1e-5 /
atol 1e-6 (test_rma_edges_gpu.py test_aggregation_backward_every_channel_path)."""
import os
import runpy
import warnings

import numpy as np
import pytest
import torch

from helpers import (DEPTH_EDGE_KS, DEPTH_EDGE_VIEWS, DEPTH_EDGES, count_mismatch, depth_last_step_facts, depth_last_step_variant,
                     depth_oracle_views, load_golden, t)
from oracle import rma_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT_TOL = dict(rtol=2e-6, atol=1e-7)
_G = {}


def _golden():
    if not _G:
        _G.update(load_golden(DEPTH_EDGES))
    return _G


def _on_device(g, device, feats=None):
    from cnrma_amd import rma
    f = t(g["features"]) if feats is None else feats
    return rma.to_nhwc(f.to(device)), t(g["proj_inv"], device), t(g["tsdf"], device)


def _geom(g, n_steps=None):
    return g["dims"], g["voxel_size"], g["origin"], g["n_steps"] if n_steps is None else n_steps


def _seeded_maps(shape, seed):
    return torch.round(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 64) / 64


# ---------------------------------------------------------------------------------------------------------------------
# rows against the reference's, all views in one call and view by view
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_rows_equal_the_reference(device, k):
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    exp, counts = g[f"depth_k{k}_rows"], [int(c) for c in g[f"depth_k{k}_counts"]]
    rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf, *_geom(g), mode="depth", select_grids=k)
    assert per_view.cpu().tolist() == counts
    miss = DEPTH_EDGE_VIEWS["miss"]
    assert counts[miss] == 0 and min(counts[:miss]) > 0 and min(counts[miss + 1:]) > 0      # the empty view lies between hit views
    assert rows.shape == exp.shape and count_mismatch(rows, exp) == 0
    lo = 0
    for v, n in enumerate(counts):
        r, pv = rma.rma_view_rows(nhwc[v:v + 1], pinv[v:v + 1], tsdf, *_geom(g), mode="depth", select_grids=k)
        assert pv.cpu().tolist() == [n] and r.shape == (n, exp.shape[1])
        assert count_mismatch(r, exp[lo:lo + n]) == 0, (k, v)
        lo += n


@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_last_sample_inside_the_grid_is_no_change(device, k):
    """the loop bound n < N - 1 against the 1 appended at N-1 (:876-878): on an all-negative TSDF, seen from one corner of the
    grid along its diagonal, the rays that stay inside for all N steps give no row (a march that multiplied the last sample
    with an "outside" 1.0 would hit there); the rays beside them hit where they leave.  Against the reference's rows."""
    from cnrma_amd import rma
    g = _golden()
    inside_no_hit, hits = depth_last_step_facts(g, k)
    assert inside_no_hit > 0 and hits > 0
    proj, tsdf = depth_last_step_variant(g)
    exp = g[f"last_step_k{k}_rows"]
    nhwc = rma.to_nhwc(t(g["features"][:1], device))
    rows, per_view = rma.rma_view_rows(nhwc, t(g["proj_inv_last_step"], device), tsdf.to(device), *_geom(g), mode="depth",
                                       select_grids=k)
    assert per_view.cpu().tolist() == [exp.shape[0]] and rows.shape == exp.shape and count_mismatch(rows, exp) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the two entry points themselves, writing into the middle of canaried buffers
# ---------------------------------------------------------------------------------------------------------------------
PAD = 64


@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_count_and_emit_write_their_outputs_and_nothing_else(device, k):
    from cnrma_amd import rma
    from cnrma_amd._lib import call, ptr, stream
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    V, H, W, C = nhwc.shape
    R = V * H * W
    dims, vs, org, N = _geom(g)
    t_one = rma.step_length(dims, vs, N)
    _, counts, dbg = depth_oracle_views(g, t(g["features"]), t(g["tsdf"]), k)
    exp_cnt = torch.cat([(d["wts"] > 0).sum(dim=1) for d in dbg]).to(torch.int32)
    exp_ws = torch.cat([d["wts"].double().sum(dim=1) for d in dbg])          # sums of at most 8 weights j/k: exact in fp64
    cnt = torch.full((R + 2 * PAD,), -7, dtype=torch.int32, device=device)
    ws = torch.full((R + 2 * PAD,), -7.0, dtype=torch.float64, device=device)
    call("cnrma_rma_depth_count_f32", ptr(pinv), ptr(tsdf), V, H, W, *dims, vs, *org, N, t_one, k,
         cnt.data_ptr() + 4 * PAD, ws.data_ptr() + 8 * PAD, stream())
    cnt_h, ws_h = cnt.cpu(), ws.cpu()
    assert torch.equal(cnt_h[PAD:PAD + R], exp_cnt) and torch.equal(ws_h[PAD:PAD + R], exp_ws)
    assert (cnt_h[:PAD] == -7).all() and (cnt_h[PAD + R:] == -7).all() and (ws_h[:PAD] == -7).all() and (ws_h[PAD + R:] == -7).all()
    M, Wd = sum(counts), 4 + C
    assert M == int(exp_cnt.sum()) == g[f"depth_k{k}_rows"].shape[0]
    off = rma.exclusive_scan(cnt[PAD:PAD + R].clone())
    assert int(off[-1]) == M
    rows = torch.full((M + 2 * PAD, Wd), -7.5, dtype=torch.float32, device=device)
    base = rows.data_ptr() + 4 * PAD * Wd
    call("cnrma_rma_depth_emit_f32", ptr(pinv), ptr(tsdf), ptr(nhwc), V, C, H, W, *dims, vs, *org, N, t_one, k, ptr(off), None,
         None, 0.0, 0.0, 0.0, base, Wd, base + 12, Wd, base + 16, Wd, 0, 0, stream())
    rows_h = rows.cpu().numpy()
    assert count_mismatch(rows_h[PAD:PAD + M], g[f"depth_k{k}_rows"]) == 0
    assert (rows_h[:PAD] == -7.5).all() and (rows_h[PAD + M:] == -7.5).all()
    # separate outputs with their own strides, a selection and the capacities of the static path: only the first `out_cap`
    # selected rows are written, each where the selection puts it
    keep = torch.from_numpy(np.random.default_rng(k).random(M) < 0.5)
    sel = torch.where(keep, torch.cumsum(keep.long(), 0) - 1, torch.tensor(-1)).to(torch.int32).to(device)
    n_keep = int(keep.sum())
    out_cap = n_keep - 3
    xyz = torch.full((n_keep + PAD, 3), -7.5, device=device)
    wcol = torch.full((n_keep + PAD,), -7.5, device=device)
    feat = torch.full((n_keep + PAD, C), -7.5, device=device)
    call("cnrma_rma_depth_emit_f32", ptr(pinv), ptr(tsdf), ptr(nhwc), V, C, H, W, *dims, vs, *org, N, t_one, k, ptr(off), ptr(sel),
         None, 0.0, 0.0, 0.0, ptr(xyz), 3, ptr(wcol), 1, ptr(feat), C, M, out_cap, stream())
    want = g[f"depth_k{k}_rows"][keep.numpy()][:out_cap]
    got = torch.cat((xyz, wcol.view(-1, 1), feat), dim=1).cpu().numpy()
    assert count_mismatch(got[:out_cap], want) == 0 and (got[out_cap:] == -7.5).all()


def test_argument_rules_return_einval(device):
    """nothing is launched: every pointer is NULL"""
    from cnrma_amd import _lib
    lib = _lib.load()
    good = dict(V=1, C=4, H=3, W=3, X=4, Y=4, Z=4, n_steps=8, k=2, sel_cap=0, out_cap=0)

    def count(**kw):
        a = dict(good, **kw)
        return lib.cnrma_rma_depth_count_f32(None, None, a["V"], a["H"], a["W"], a["X"], a["Y"], a["Z"], 0.04, 0.0, 0.0, 0.0,
                                             a["n_steps"], 0.01, a["k"], None, None, None)

    def emit(**kw):
        a = dict(good, **kw)
        return lib.cnrma_rma_depth_emit_f32(None, None, None, a["V"], a["C"], a["H"], a["W"], a["X"], a["Y"], a["Z"], 0.04, 0.0, 0.0,
                                            0.0, a["n_steps"], 0.01, a["k"], None, None, None, 0.0, 0.0, 0.0, None, 0, None, 0, None,
                                            0, a["sel_cap"], a["out_cap"], None)

    bad = [dict(k=-1), dict(n_steps=0), dict(n_steps=-3)]
    bad += [{d: z} for d in ("V", "H", "W", "X", "Y", "Z") for z in (0, -1)]
    for kw in bad:
        assert count(**kw) == _lib.EINVAL, kw
        assert emit(**kw) == _lib.EINVAL, kw
    for kw in (dict(C=0), dict(C=-4), dict(sel_cap=-1), dict(out_cap=-1)):
        assert emit(**kw) == _lib.EINVAL, kw


# ---------------------------------------------------------------------------------------------------------------------
# scene aggregate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_scene_aggregate_equals_the_oracle(device, k):
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    dims, vs, org, N = _geom(g)
    exp = O.aggregate_rma(t(g["projection"]), t(g["features"]), t(g["tsdf"]), dims, vs, org, g["stride"], N, mode="depth",
                          select_grids=k, proj_inv=t(g["proj_inv"]))
    assert count_mismatch(exp, g[f"depth_k{k}_points"]) == 0                     # the oracle's is the reference's
    pts, info = rma.aggregate_rows(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
    pts = pts.cpu().numpy()
    assert info["M"] == exp.shape[0] and pts.shape == tuple(exp.shape)
    assert count_mismatch(pts[:, :3], exp[:, :3]) == 0
    np.testing.assert_allclose(pts[:, 3:], exp[:, 3:].numpy(), **FEAT_TOL)
    # with an offset and an explicit mask: the selected rows, in order
    M = exp.shape[0]
    mask = np.random.default_rng(10 + k).random(M) < 0.4
    offset = (0.37, -1.21, 0.05)
    c, f, info = rma.aggregate_points(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k, offset=offset, mask=mask)
    ec, ef = O.select_rows(exp, offset, mask)
    assert info["M"] == M and info["M_selected"] == int(mask.sum()) == c.shape[0] > 0
    assert count_mismatch(c, ec) == 0
    np.testing.assert_allclose(f.cpu().numpy(), ef.numpy(), **FEAT_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# every channel path of emit_row: float4 when C, the row stride and both addresses allow it, scalar otherwise
# ---------------------------------------------------------------------------------------------------------------------
# raw rows have stride 4 + C and features at column 4: 16-byte aligned for C % 4 == 0 (12, 40, 96, 256: float4), not for 3, 5;
# the aggregate's rows have stride C: float4 for 12, 40, 96, 256, scalar for 3 and 5
@pytest.mark.parametrize("C", [3, 5, 12, 40, 96, 256])
def test_emission_every_channel_path(device, C):
    from cnrma_amd import rma
    g = _golden()
    V, _, H, W = g["features"].shape
    f = _seeded_maps((V, C, H, W), 500 + C)
    nhwc, pinv, tsdf = _on_device(g, device, f)
    dims, vs, org, N = _geom(g)
    for k in (0, 3):
        exp, counts, _ = depth_oracle_views(g, f, t(g["tsdf"]), k)
        assert counts == [int(c) for c in g[f"depth_k{k}_counts"]]            # same geometry: the fixture's kept set
        rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        assert per_view.cpu().tolist() == counts and count_mismatch(rows, exp) == 0, (C, k)
        ep = O.aggregate_rma(t(g["projection"]), f, t(g["tsdf"]), dims, vs, org, g["stride"], N, mode="depth", select_grids=k,
                             proj_inv=t(g["proj_inv"])).numpy()
        pts, _ = rma.aggregate_rows(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        pts = pts.cpu().numpy()
        assert pts.shape == ep.shape and count_mismatch(pts[:, :3], ep[:, :3]) == 0
        np.testing.assert_allclose(pts[:, 3:], ep[:, 3:], **FEAT_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# ray counts around a wave (64) and a block (256)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257)])
def test_ray_counts_around_a_wave_and_a_block(device, H, W):
    from cnrma_amd import rma
    g = _golden()
    v = DEPTH_EDGE_VIEWS["inside"]
    H0, W0 = g["features"].shape[-2:]
    proj = t(g["projection"][v:v + 1]).clone()                   # the inside camera, re-scaled to an H x W map
    proj[:, 0] *= W / W0
    proj[:, 1] *= H / H0
    pinv = rma.projection_inverse(proj, g["stride"])
    f = _seeded_maps((1, 4, H, W), 600 + H * W)
    dims, vs, org, N = _geom(g)
    exp, counts, dbg = depth_oracle_views(g, f, t(g["tsdf"]), 2, projection=proj, proj_inv=pinv)
    rows, per_view = rma.rma_view_rows(rma.to_nhwc(f.to(device)), pinv.to(device), t(g["tsdf"], device), dims, vs, org, N,
                                       mode="depth", select_grids=2)
    assert per_view.cpu().tolist() == counts and rows.shape == exp.shape and count_mismatch(rows, exp) == 0
    if H * W >= 63:
        assert 0 < int(dbg[0]["hit"].sum()) and counts[0] > 0


# ---------------------------------------------------------------------------------------------------------------------
# short marches
# ---------------------------------------------------------------------------------------------------------------------
def test_one_step_march_has_no_product_and_no_row(device):
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    dims, vs, org, _ = _geom(g)
    for k in (0, 4):
        exp, counts, _ = depth_oracle_views(g, t(g["features"]), t(g["tsdf"]), k, n_steps=1)
        assert sum(counts) == 0
        rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf, dims, vs, org, 1, mode="depth", select_grids=k)
        assert rows.shape == exp.shape and per_view.cpu().tolist() == counts
        with pytest.raises(TypeError):
            O.aggregate_rma(t(g["projection"]), t(g["features"]), t(g["tsdf"]), dims, vs, org, g["stride"], 1, mode="depth",
                            select_grids=k, proj_inv=t(g["proj_inv"]))
        with pytest.raises(TypeError):
            rma.aggregate_rows(nhwc, pinv, tsdf, dims, vs, org, 1, mode="depth", select_grids=k)


@pytest.mark.parametrize("N", [2, 3])
def test_short_march_at_k4_masks_almost_every_slot(device, N):
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    dims, vs, org, _ = _geom(g)
    exp, counts, dbg = depth_oracle_views(g, t(g["features"]), t(g["tsdf"]), 4, n_steps=N)
    hits = sum(int(d["hit"].sum()) for d in dbg)
    assert hits > 0 and sum(counts) == N * hits                  # of the 8 slots of a hit ray exactly those in [0, N) stay
    rows, per_view = rma.rma_view_rows(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=4)
    assert per_view.cpu().tolist() == counts and count_mismatch(rows, exp) == 0
    ep = O.aggregate_rma(t(g["projection"]), t(g["features"]), t(g["tsdf"]), dims, vs, org, g["stride"], N, mode="depth",
                         select_grids=4, proj_inv=t(g["proj_inv"])).numpy()
    pts, _ = rma.aggregate_rows(nhwc, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=4)
    pts = pts.cpu().numpy()
    assert pts.shape == ep.shape and count_mismatch(pts[:, :3], ep[:, :3]) == 0
    np.testing.assert_allclose(pts[:, 3:], ep[:, 3:], **FEAT_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit maps are widened (_March): bit for bit the run on their fp32 widening
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_maps_equal_their_widening(device, dtype):
    from cnrma_amd import rma
    g = _golden()
    V, _, H, W = g["features"].shape
    f16 = torch.randn(V, 8, H, W, generator=torch.Generator().manual_seed(700)).to(dtype)
    nhwc16 = rma.to_nhwc(f16.to(device), keep_dtype=True)
    assert nhwc16.dtype == dtype
    _, pinv, tsdf = _on_device(g, device)
    dims, vs, org, N = _geom(g)
    wide = nhwc16.float()
    for k in (0, 2):
        a, pa = rma.rma_view_rows(nhwc16, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        b, pb = rma.rma_view_rows(wide, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        assert torch.equal(pa, pb) and a.shape == b.shape and count_mismatch(a, b) == 0
        exp, counts, _ = depth_oracle_views(g, f16.float(), t(g["tsdf"]), k)
        assert pa.cpu().tolist() == counts and count_mismatch(a, exp) == 0
        pa_, _ = rma.aggregate_rows(nhwc16, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        pb_, _ = rma.aggregate_rows(wide, pinv, tsdf, dims, vs, org, N, mode="depth", select_grids=k)
        assert count_mismatch(pa_, pb_) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the static trace (device-side row count, capacity-guarded emission), eager and captured, at k = 3 and 4
# ---------------------------------------------------------------------------------------------------------------------
def _static_trace(plan, args, k, max_points, offset):
    from cnrma_amd import plan as P
    from cnrma_amd import rma
    plan.begin_static()
    with P.using(plan), torch.no_grad():
        coords, feats, n_sel, info = rma.aggregate_points_static(*args, offset=offset, max_points=max_points, seed=5, mode="depth",
                                                                 select_grids=k)
        status = plan.status(coords.device)
    plan.end_static()
    return coords, feats, n_sel, info["sel"], info["M"], status


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("max_points", [None, 700], ids=["all", "max700"])
@pytest.mark.parametrize("k", [3, 4])
def test_static_trace_equals_the_oracle(device, k, max_points, capture):
    from cnrma_amd import plan as P
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    dims, vs, org, N = _geom(g)
    args = (nhwc, pinv, tsdf, dims, vs, org, N)
    offset = (0.37, -1.21, 0.05)
    exp = O.aggregate_rma(t(g["projection"]), t(g["features"]), t(g["tsdf"]), dims, vs, org, g["stride"], N, mode="depth",
                          select_grids=k, proj_inv=t(g["proj_inv"]))
    M = exp.shape[0]
    assert max_points is None or max_points < M
    plan = P.Plan()
    with P.using(plan):                                        # calibration: the eager pass records the row count
        rma.aggregate_points(*args, mode="depth", select_grids=k)
    assert plan.sizes == [M]
    out = _static_trace(plan, args, k, max_points, offset)     # first static run: outside capture (it builds the plan's constants)
    if capture:
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.graph(graph, stream=side):
            out = _static_trace(plan, args, k, max_points, offset)
        for o in out[:4]:
            if o is not None:
                o.fill_(-1)                                    # a replay must write everything it reports
        graph.replay()
        torch.cuda.synchronize(device)
    coords, feats, n_sel, sel, m_dev, status = out
    n = int(n_sel)
    assert int(status) == 0 and int(m_dev) == M and n == (M if max_points is None else max_points)
    chosen = sel[:M].cpu().numpy()
    rows = np.nonzero(chosen >= 0)[0]
    assert len(rows) == n and (chosen[rows] == np.arange(n)).all()                  # the selected rows, in order
    ec, ef = O.select_rows(exp[torch.from_numpy(rows)], offset)
    assert count_mismatch(coords[:n], ec) == 0
    np.testing.assert_allclose(feats[:n].cpu().numpy(), ef.numpy(), **FEAT_TOL)


def test_static_trace_reports_a_scene_that_outgrows_its_plan(device):
    """a plan calibrated on a quarter of the rows: the emission stops at its capacities and the status word says so"""
    from cnrma_amd import plan as P
    from cnrma_amd import rma
    g = _golden()
    nhwc, pinv, tsdf = _on_device(g, device)
    args = (nhwc, pinv, tsdf, *_geom(g))
    M = g["depth_k4_points"].shape[0]
    plan = P.Plan(margin=1.0, slack=0)
    plan.sizes = [M // 4]
    coords, feats, n_sel, sel, m_dev, status = _static_trace(plan, args, 4, None, (0.0, 0.0, 0.0))
    cap = coords.shape[0]
    assert cap < M and int(m_dev) == M and int(status) > 0
    assert count_mismatch(coords[:cap], g["depth_k4_points"][:cap, :3]) == 0       # what fits is what the full run gives


# ---------------------------------------------------------------------------------------------------------------------
# training in depth mode: the detection loss's gradient reaches the 2D feature maps (reference :947 indexes them)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
def test_depth_mode_gradient_reaches_the_feature_maps(device, tmp_path, k):
    """through the detector's aggregate_2d_features_ray_marching (300 steps, as the plugin marches) with
    ray_marching_type="depth": points_detection carries autograd history, and the gradient of (points[:, 3:] * g).sum() with
    respect to the maps equals autograd through the oracle with the maps in float64 at rtol 1e-5 / atol 1e-6 -- the bar of
    the NeuS gradient test; exactly zero on pixels whose ray has no hit; the backward reads nothing back to the host"""
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_model
    from cnrma_amd import rma
    g = _golden()
    dims, vs, org, _ = _geom(g)
    V, C, H, W = g["features"].shape
    cfg = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))
    m = dict(cfg["model"])
    m.update(backbone2d=None, feature_2d=None, backbone_3d=None, tsdf_head=None)
    m.update(save_path=str(tmp_path / "r"), voxel_dim_test=list(dims), voxel_dim_train=list(dims), origin=list(org), max_points=None,
             backbone2d_stride=g["stride"], voxel_size=vs, use_feature_transform=False, ray_marching_type="depth", depth_points=k,
             neus_threshold=None, detection_backbone=dict(type="FCAF3DBackbone", in_channels=C, depth=14))
    model = build_model(m).to(device).train()
    model.voxel_dim = list(dims)
    f_cpu = torch.randn(V, C, H, W, generator=torch.Generator().manual_seed(800 + k))
    proj, tsdf = t(g["projection"]), t(g["tsdf"])
    pinv = rma.projection_inverse(proj, g["stride"])             # what the plugin computes; the oracle marches on the same
    f64 = f_cpu.double().requires_grad_(True)
    ref_pts = O.aggregate_rma(proj, f64, tsdf, dims, vs, org, g["stride"], 300, mode="depth", select_grids=k, proj_inv=pinv)
    gr = torch.randn(ref_pts.shape[0], C, generator=torch.Generator().manual_seed(900 + k))
    (ref_pts[:, 3:] * gr.double()).sum().backward()
    ref = f64.grad.numpy()
    f_gpu = f_cpu.to(device).requires_grad_(True)
    model.aggregate_2d_features_ray_marching(proj.to(device).unsqueeze(1), f_gpu.unsqueeze(1), tsdf.to(device).view(1, 1, *dims))
    pts = model.points_detection[0]
    assert pts.requires_grad
    assert pts.shape == ref_pts.shape and count_mismatch(pts[:, :3].detach(), ref_pts[:, :3].detach().float()) == 0
    np.testing.assert_allclose(pts[:, 3:].detach().cpu().numpy(), ref_pts[:, 3:].detach().numpy(), rtol=1e-5, atol=1e-6)
    loss = (pts[:, 3:] * gr.to(device)).sum()
    torch.cuda.synchronize(device)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # "a prototype feature": said once when the mode is set
        torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not [w for w in seen if "synchroniz" in str(w.message)], [str(w.message) for w in seen]
    got = f_gpu.grad.cpu().numpy()
    print(f"depth gradient k={k}: max |got - ref| = {np.abs(got - ref).max():.3e}, max |ref| = {np.abs(ref).max():.3e}")
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    assert float(np.abs(got).sum()) > 0
    _, _, dbg = depth_oracle_views(g, f_cpu, tsdf, k, n_steps=300, proj_inv=pinv)
    none = ~torch.stack([d["hit"] for d in dbg]).view(V, H, W).numpy()
    assert none.any() and (~none).any() and (got.transpose(0, 2, 3, 1)[none] == 0).all()
    assert (got[ref == 0] == 0).all()


@pytest.mark.parametrize("how", ["mask", "max_points"])
@pytest.mark.parametrize("k", [0, 3])
def test_depth_gradient_with_a_selection(device, k, how):
    """rma.AggregatePoints(mode="depth") with an explicit mask / a numpy-drawn max_points subset, at the fixture's 40 steps:
    only the selected rows carry gradient, each into its own ray's pixel (the ray of a selected row is found on the device
    from the per-ray counts and the selection index).  Same reference and bar as above."""
    from cnrma_amd import rma
    g = _golden()
    dims, vs, org, N = _geom(g)
    V, C, H, W = g["features"].shape
    proj, tsdf, pinv = t(g["projection"]), t(g["tsdf"]), t(g["proj_inv"])
    f64 = torch.randn(V, C, H, W, generator=torch.Generator().manual_seed(820 + k)).double().requires_grad_(True)
    pts = O.aggregate_rma(proj, f64, tsdf, dims, vs, org, g["stride"], N, mode="depth", select_grids=k, proj_inv=pinv)
    M = pts.shape[0]
    n_keep = M // 3
    np.random.seed(40 + k)
    mask = O.sample_mask_numpy(M, n_keep) if how == "max_points" else np.random.default_rng(k).random(M) < 0.3
    sel = pts[torch.from_numpy(mask)][:, 3:]
    gr = torch.randn(sel.shape, generator=torch.Generator().manual_seed(830 + k))
    (sel * gr.double()).sum().backward()
    ref = f64.grad.numpy()
    f_gpu = f64.detach().float().to(device).requires_grad_(True)
    np.random.seed(40 + k)                                       # the numpy sampler draws the oracle's subset again
    coords, feats = rma.AggregatePoints.apply(f_gpu, pinv.to(device), tsdf.to(device), dims, vs, org, N, 0.0, (0.0, 0.0, 0.0),
                                              n_keep if how == "max_points" else None, "numpy",
                                              mask if how == "mask" else None, "depth", k)
    assert feats.shape == sel.shape and count_mismatch(coords, pts[torch.from_numpy(mask)][:, :3].detach().float()) == 0
    np.testing.assert_allclose(feats.detach().cpu().numpy(), sel.detach().numpy(), rtol=1e-5, atol=1e-6)
    (feats * gr.to(device)).sum().backward()
    got = f_gpu.grad.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    assert float(np.abs(got).sum()) > 0 and (ref == 0).any() and (got[ref == 0] == 0).all()


def test_depth_mode_train_step_reaches_the_feature_maps(device, tmp_path):
    """train_step of the registered detector with ray_marching_type="depth": the detection loss's gradient arrives at the 2D
    feature maps, finite and non-zero (it stopped at the aggregation before: nothing raised, the maps just got none)"""
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_model
    from cnrma_amd import synth
    sc = synth.make_scene("tiny", seed=6)
    C = sc["features"].shape[2]
    cfg = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))
    m = dict(cfg["model"])
    m.update(backbone2d=None, feature_2d=None, backbone_3d=None, tsdf_head=None)
    m.update(save_path=str(tmp_path / "r"), voxel_dim_test=list(sc["dims"]), voxel_dim_train=list(sc["dims"]), max_points=1000,
             use_feature_transform=False, ray_marching_type="depth", depth_points=2, neus_threshold=None,
             detection_backbone=dict(type="FCAF3DBackbone", in_channels=C, depth=14))
    torch.manual_seed(2)
    np.random.seed(3)
    model = build_model(m)
    model.detection_backbone.init_weights()
    model.detection_head.init_weights()
    model = model.to(device).train()
    dims = np.array(sc["dims"], dtype=np.float32) * 0.04
    boxes = torch.tensor([[0.35 * dims[0], 0.4 * dims[1], 0.1 * dims[2], 0.5, 0.4, 0.5, 0.0],
                          [0.65 * dims[0], 0.6 * dims[1], 0.2 * dims[2], 0.4, 0.6, 0.4, 0.0]], device=device)
    feats = sc["features"][:, 0].to(device).requires_grad_(True)
    tsdf = sc["tsdf"] - 0.5              # the synthetic room's TSDF is positive throughout (0.17 .. 1): moved so that it changes sign
    assert float(tsdf.min()) < 0 < float(tsdf.max())
    data = dict(features=[feats], projection=[sc["projection"][:, 0].to(device)], tsdf=tsdf.to(device),
                offset=[torch.zeros(3, device=device)], gt_bboxes_3d=[boxes], gt_labels_3d=[torch.tensor([1, 3], device=device)])
    out = model.train_step(dict(data), None)
    assert model.points_detection[0].requires_grad and model.points_detection[0].shape[0] > 1000
    out["loss"].backward()
    assert torch.isfinite(out["loss"]) and torch.isfinite(feats.grad).all() and float(feats.grad.abs().sum()) > 0
