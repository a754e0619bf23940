"""tests/head_select_model.py checked on the CPU: the model of the FCAF3D head's selection rule against torch.topk where that is
defined, its tie rule, and the promises of the input builders that tests/test_head_select_gpu.py relies on."""
import numpy as np
import pytest
import torch

import head_select_model as M
from oracle import sparse_oracle as SO

KS = (64, 1000)


def _counts(k):
    return (0, 1, k - 1, k, k + 1, 2 * k + 3)


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("counts", [(1,), (63,), (64,), (65,), (131,), (65, 64), (131, 0, 63), (63, 0, 131)])
def test_model_equals_torch_topk_without_ties(counts, k):
    rng = np.random.RandomState(sum(counts) + k)
    n = sum(counts)
    scene = np.repeat(np.arange(len(counts)), counts)
    scores = rng.permutation(n).astype(np.float64) / n                  # all distinct
    kept, cut, r0 = [], M.cut_rows(scene, scores, k, len(counts)), 0
    for b, nb in enumerate(counts):
        mine = torch.from_numpy(scores[r0:r0 + nb])
        if nb > k:
            idx = torch.topk(mine, k)[1].numpy() + r0
            assert np.array_equal(cut[b], idx)
            kept.append(np.sort(idx))
        else:
            assert np.array_equal(cut[b], np.arange(r0, r0 + nb))
            kept.append(np.arange(r0, r0 + nb))
        r0 += nb
    assert np.array_equal(M.prune_rows(scene, scores, k, len(counts)), np.concatenate(kept))


def test_model_keeps_the_lowest_indices_of_a_tie():
    #                  0    1    2    3    4    5    6    7 | 8    9   10
    scores = np.array([.5, .9, .5, .5, .1, .9, .5, .5, .7, .7, .7])
    scene = np.array([0] * 8 + [1] * 3)
    assert M.cut_rows(scene, scores, 4)[0].tolist() == [1, 5, 0, 2]
    assert M.cut_rows(scene, scores, 4)[1].tolist() == [8, 9, 10]          # not above the cut: row order
    assert M.cut_rows(scene, scores, 2)[1].tolist() == [8, 9]
    assert M.prune_rows(scene, scores, 4).tolist() == [0, 1, 2, 5, 8, 9, 10]
    assert M.prune_rows(scene, scores, 2).tolist() == [1, 5, 8, 9]
    assert M.prune_rows(scene, scores, -1).tolist() == list(range(11))
    for nms_pre in (0, -1):                                                 # no cut: everything, in row order
        assert [r.tolist() for r in M.cut_rows(scene, scores, nms_pre)] == [list(range(8)), [8, 9, 10]]
    assert [len(r) for r in M.cut_rows(scene[:8], scores[:8], 4, n_scenes=3)] == [4, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the builders
# ---------------------------------------------------------------------------------------------------------------------
def _ranks(keys):
    """keys by descending rank: the sequence a scene was built from"""
    return np.sort(keys)[::-1]


@pytest.mark.parametrize("pattern", M.PATTERNS)
@pytest.mark.parametrize("k", KS + (1500,))
def test_scene_groups_put_the_ties_where_they_belong(k, pattern):
    rng = np.random.RandomState(k)
    for n in _counts(k):
        keys = M.scene_groups(n, k, pattern, rng)
        assert keys.shape == (n,)
        r = _ranks(keys)
        fits = n >= k + 2
        if pattern == "equal":
            assert len(np.unique(keys)) == min(n, 1)
        elif pattern == "straddle5" and fits:
            g = r[k - 3]
            assert (r[k - 3:k + 2] == g).all() and (keys == g).sum() == 5 and M.ZERO < g < M.ONE
        elif pattern == "zeros" and n > k:
            assert (r[k - 2:] == M.ZERO).all() and (keys == M.ZERO).sum() == n - k + 2 and r[k - 3] > M.ZERO
        elif pattern == "ones" and fits:
            assert (r[:k + 2] == M.ONE).all() and (keys == M.ONE).sum() == k + 2
        else:
            assert keys.min(initial=0) >= 0 and keys.max(initial=0) < M.PALETTE
            if n <= M.PALETTE - 3:
                assert len(np.unique(keys)) == n                               # no ties at all
            else:
                assert np.bincount(keys).max() == -(-n // (M.PALETTE - 3))


@pytest.mark.parametrize("pattern", M.PATTERNS)
@pytest.mark.parametrize("k", KS)
def test_cut_levels_keep_their_promises(k, pattern):
    """per-scene counts as asked; within a scene rows have the same float64 max score exactly when they have the same key, and
    then bit-identical logits; distinct max scores differ by at least GAP; the saturated groups are exactly 0 and 1 in float32"""
    counts = (2 * k + 3, 0, k - 1, k, k + 1, 1)
    lv = M.cut_level(counts, k, pattern, 18, seed=k)
    assert np.bincount(lv["scene"], minlength=len(counts)).tolist() == list(counts)
    assert (np.diff(lv["scene"]) >= 0).all()                                    # scene-major
    assert lv["cen"].dtype == np.float32 and lv["cls"].dtype == np.float32 and lv["cls"].shape == (sum(counts), 18)
    logits = np.concatenate((lv["cen"], lv["cls"]), axis=1).view(np.uint32)
    values = np.unique(lv["score"])
    assert np.diff(values).min(initial=1.0) >= M.GAP
    by_key = {}
    for g in np.unique(lv["keys"]):
        rows = np.nonzero(lv["keys"] == g)[0]
        assert (logits[rows] == logits[rows[0]]).all()
        assert (lv["score"][rows] == lv["score"][rows[0]]).all()
        by_key[int(g)] = lv["score"][rows[0]]
    assert len(set(by_key.values())) == len(by_key)                             # different keys, different scores ...
    ordered = sorted(by_key)
    assert all(by_key[a] < by_key[b] for a, b in zip(ordered, ordered[1:]))     # ... ordered like the keys
    s32 = (M.sigmoid64(lv["cls"]) * M.sigmoid64(lv["cen"])).astype(np.float32).max(axis=1)
    assert (s32[lv["keys"] == M.ZERO] == 0).all() and (s32[lv["keys"] == M.ONE] == 1).all()
    assert (lv["score"][lv["keys"] == M.ONE] == 1.0).all()
    if pattern == "zeros":
        assert (lv["keys"] == M.ZERO).sum() == (k + 5) + 3                      # scenes of 2k+3 and k+1 rows
    if pattern == "ones":
        assert (lv["keys"] == M.ONE).sum() == k + 2


def test_every_palette_value_is_separated():
    cen, cls = M.head_logits(np.arange(M.PALETTE), 18)
    s = M.class_scores64(cls, cen).max(axis=1)
    assert np.diff(s).min() >= M.GAP and s[0] >= 3e-3 and s[-1] <= 1 - 5e-3
    assert (M.class_scores64(cls, cen).argmax(axis=1) == np.arange(M.PALETTE) % 18).all()


@pytest.mark.parametrize("n_reg,yaw", [(6, "fcaf3d"), (8, "fcaf3d"), (8, "sin-cos"), (7, "naive")])
def test_identity_rows_decode_to_their_index(n_reg, yaw):
    pts, box = M.identity_rows(3000, n_reg)
    out = SO.decode_boxes(torch.from_numpy(pts), torch.from_numpy(box), yaw).numpy()
    assert out.dtype == np.float32 and np.array_equal(out[:, 0], np.arange(3000)) and np.isfinite(out).all()


@pytest.mark.parametrize("off_site", [False, True], ids=["on_site", "off_site"])
@pytest.mark.parametrize("pattern", M.PATTERNS)
def test_prune_levels_interpolate_to_their_values(pattern, off_site):
    """the oracle's interpolation of the built score field at the built queries is the group's value exactly; values of different
    groups differ by at least GAP; coordinates are unique, on their lattices and scene-major"""
    T, s = 64, 8
    counts = (2 * T + 3, 0, T - 1, T + 1)
    lv = M.prune_level(counts, T, pattern, s, seed=3, off_site=off_site)
    assert np.bincount(lv["scene"], minlength=4).tolist() == list(counts)
    for c, lattice in ((lv["coords"], s), (lv["score_coords"], 2 * s)):
        assert (c[:, 1:] % lattice == 0).all() and len(np.unique(c, axis=0)) == len(c) and (np.diff(c[:, 0]) >= 0).all()
        assert np.abs(c[:, 1:]).max() < 32000
    if off_site:
        assert (lv["coords"][:, 1] % (2 * s) == s).all() and (lv["coords"][:, 2] % (2 * s) == s).any()
    got = SO.interpolate(lv["score_coords"], lv["score"], 2 * s, lv["coords"]).reshape(-1)
    assert np.array_equal(got, lv["value"])
    assert np.array_equal(lv["value"], M.prune_value(lv["keys"]).astype(np.float64))
    assert np.diff(np.unique(lv["value"])).min(initial=1.0) >= M.GAP
    assert np.array_equal(lv["feats"][:, 0], np.arange(sum(counts)))
