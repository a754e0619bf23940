"""The depth-mode edge fixture (tests/golden/rma_depth_edges.npz, make_golden.py run_depth_edges) on the CPU: the oracle
reproduces the reference's rows of every view and the scene aggregate bit for bit for select_grids = 0..4, and the fixture
holds the edges it is for (re-derived from its inputs: helpers.depth_edge_facts)."""
import numpy as np
import pytest
import torch

from helpers import (DEPTH_EDGE_KS, DEPTH_EDGE_VIEWS, DEPTH_EDGES, count_mismatch, depth_edge_facts, depth_last_step_facts,
                     depth_last_step_variant, depth_oracle_views, load_golden, t)
from oracle import rma_oracle as O


@pytest.fixture(scope="module")
def g():
    return load_golden(DEPTH_EDGES)


def test_fixture_holds_its_edges(g):
    f = depth_edge_facts(g)
    assert f.pop("miss_hits") == 0
    assert all(n > 0 for n in f.values()), f
    # the slots below 0 are -1, -2 and -3 (first changes at steps 0, 1 and 2 under k = 4); the planted values are in the TSDF
    _, _, dbg = depth_oracle_views(g, t(g["features"]), t(g["tsdf"]), 4)
    i = dbg[DEPTH_EDGE_VIEWS["inside"]]
    assert set(i["sel"][i["hit"]].unique().tolist()) >= {-3, -2, -1}
    tsdf = g["tsdf"]
    assert np.isnan(tsdf).any() and (tsdf == 1.0).any()
    assert ((tsdf == 0) & ~np.signbit(tsdf)).any() and ((tsdf == 0) & np.signbit(tsdf)).any()
    assert any(o != 0 for o in g["origin"]) and g["n_steps"] == 40


@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_oracle_rows_equal_the_reference(g, k):
    feats, tsdf = t(g["features"]), t(g["tsdf"])
    rows, counts, _ = depth_oracle_views(g, feats, tsdf, k)
    assert counts == list(g[f"depth_k{k}_counts"])
    assert counts[DEPTH_EDGE_VIEWS["miss"]] == 0 and min(c for v, c in enumerate(counts) if v != DEPTH_EDGE_VIEWS["miss"]) > 1
    assert rows.shape == g[f"depth_k{k}_rows"].shape and count_mismatch(rows, g[f"depth_k{k}_rows"]) == 0
    # view by view through the quirk path too (no view keeps exactly one row: nothing is dropped)
    for v in range(feats.shape[0]):
        ps = O.scale_projection(t(g["projection"][v]), g["stride"])
        r = O.rma_depth_view(ps, feats[v], tsdf, g["dims"], g["voxel_size"], g["origin"], g["n_steps"], k,
                             o_d=O.ray_params(ps, feats.shape[2], feats.shape[3], t(g["proj_inv"][v])))
        lo = sum(counts[:v])
        assert (r is None) == (counts[v] == 0)
        if r is not None:
            assert count_mismatch(r, g[f"depth_k{k}_rows"][lo:lo + counts[v]]) == 0


@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_oracle_aggregate_equals_the_reference(g, k):
    pts = O.aggregate_rma(t(g["projection"]), t(g["features"]), t(g["tsdf"]), g["dims"], g["voxel_size"], g["origin"], g["stride"],
                          g["n_steps"], mode="depth", select_grids=k, proj_inv=t(g["proj_inv"]))
    exp = g[f"depth_k{k}_points"]
    assert pts.shape == exp.shape and count_mismatch(pts, exp) == 0
    assert count_mismatch(exp[:, :3], g[f"depth_k{k}_rows"][:, :3]) == 0          # the aggregate keeps the rows' places


@pytest.mark.parametrize("k", DEPTH_EDGE_KS)
def test_last_sample_inside_the_grid_is_no_change(g, k):
    """rays whose N samples all lie in negative voxels give no row: the product appended at N-1 is 1 (:876-878)"""
    inside_no_hit, hits = depth_last_step_facts(g, k)
    assert inside_no_hit > 0 and hits > 0
    proj, tsdf = depth_last_step_variant(g)
    rows, counts, dbg = depth_oracle_views(g, t(g["features"][:1]), tsdf, k, projection=proj, proj_inv=t(g["proj_inv_last_step"]))
    exp = g[f"last_step_k{k}_rows"]
    assert rows.shape == exp.shape and count_mismatch(rows, exp) == 0
    assert (tsdf < 0).all() and int(dbg[0]["best"][dbg[0]["hit"]].max()) <= g["n_steps"] - 2


def test_pinned_inverse_is_this_hosts_inverse_up_to_rounding(g):
    """proj_inv is an input of the fixture (LAPACK's inverse is not bit-stable across hosts); it is the inverse"""
    for v in range(g["projection"].shape[0]):
        ps = O.scale_projection(t(g["projection"][v]), g["stride"])
        P4 = torch.cat((ps, torch.tensor([[0.0, 0.0, 0.0, 1.0]])), dim=0).double()
        err = (P4 @ t(g["proj_inv"][v]).double() - torch.eye(4, dtype=torch.float64)).abs().max()
        assert float(err) < 1e-3
