"""The discrete selection of the FCAF3D head -- the top-k pruning of the neck and the pre-NMS cut -- on every path that states it,
row for row against tests/head_select_model.py.

  pruning:  FCAF3DHead._prune  eager with one scene / with several, static trace with B <= 1 / B > 1 under plan flags
            False, None (prune) and True (skip)
  cut:      _get_bboxes_single (through get_bboxes), get_bboxes_fused, get_bboxes_static (flags True / False / None),
            get_bboxes_static_multi

The inputs are synthetic (head_select_model: score values at least 1e-3 apart, intended ties bit-identical), and every row names
itself -- points[i] = (i, 0, 0) under a bbox_pred of equal opposite distances, so box[:, 0] == i; pruned features hold the row
index --, so membership and order are compared exactly, as integers.  Scores and boxes of the chosen rows are compared bit for bit
with sparse.select_decode on the same ids, the scores with float64 within the 1e-6 of test_post_edges_gpu.py::
test_scores_at_saturating_logits and the boxes within the 1e-5 of test_decode_entries_against_the_reference_vectors.

Counts per scene and level are 0, 1, k-1, k, k+1 and 2k+3 around the cut k (64; 1000, the shipped nms_pre; 1500 for the pruning,
beyond the 1024 of topk_indices' one-workgroup sort), alone and mixed in one scene-major row set.  The static forms get capacity
tensors whose dead rows are poison (3e38 or NaN; coordinates that copy live rows), run under a hand-made plan, twice in the same
buffers with two live counts.  Each path equals the model exactly, so the paths equal one another; one test says so directly."""
import functools
import zlib

import numpy as np
import pytest
import torch

import head_select_model as M
from helpers import capacity_tensor, poison_coords, poison_rows
from oracle import sparse_oracle as SO

pytestmark = pytest.mark.gpu

N_CLS = 18
TS = 8                                                    # tensor stride of the row sets
MODES = [(6, "fcaf3d"), (8, "fcaf3d"), (8, "sin-cos")]
POISONS = [3e38, float("nan")]
CAPS = ["plus37", "double"]


def _seed(*what):
    return zlib.crc32(repr(what).encode()) & 0x7FFFFFFF


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _capacity(live, mode):
    return live + 37 if mode == "plus37" else max(2 * live, live + 1)


@functools.lru_cache(maxsize=None)
def _head(n_reg, yaw):
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    return FCAF3DHead(N_CLS, (8, 8, 8, 8), 8, n_reg, 0.01, -1, None, yaw_parametrization=yaw, test_cfg=dict(nms_pre=0)).eval()


def _cut_head(n_reg, yaw, nms_pre):
    head = _head(n_reg, yaw)
    head.test_cfg["nms_pre"] = nms_pre
    return head


def _prune_head(T):
    head = _head(6, "fcaf3d")
    head.pts_threshold = T
    return head


def _static(plan, device, fn):
    """fn() as a static trace under the hand-made plan: (its result, the plan's status word as an int)"""
    from cnrma_amd import plan as P
    plan.begin_static()
    with P.using(plan), torch.no_grad():
        out = fn()
        status = plan.status(device)
    plan.end_static()
    return out, int(status.cpu()[0])


def _plan(flags):
    from cnrma_amd import plan as P
    p = P.Plan()
    p.flags, p.sizes = list(flags), []
    return p


# =====================================================================================================================
# the pre-NMS cut
# =====================================================================================================================
def _layouts(k):
    """rows per scene, for each of four levels"""
    L = {"b1a": [(2 * k + 3,), (k + 1,), (k,), (k - 1,)],
         "b1b": [(k,), (1,), (0,), (k + 1,)],
         "b2": [(k + 1, k), (k - 1, 2 * k + 3), (k, k), (1, 0)],
         "b3": [(2 * k + 3, 0, k - 1), (k, k + 1, 1), (0, k - 1, k), (k + 1, 2 * k + 3, 0)]}
    L["b2r"] = [c[::-1] for c in L["b2"]]
    L["b3r"] = [c[::-1] for c in L["b3"]]
    return L


# (layout, k, pattern, nms_pre)
CUT_CASES = [(lay, k, "plain", k) for k in (64, 1000) for lay in ("b1a", "b1b", "b2", "b3", "b3r")] \
    + [(lay, k, pat, k) for k in (64, 1000) for lay in ("b1a", "b3") for pat in M.PATTERNS[1:]] \
    + [("b1a", 64, "plain", 0), ("b3", 64, "plain", 0), ("b2", 64, "equal", 0)]
B1_CASES = [c for c in CUT_CASES if c[0].startswith("b1")]
OTHER = {"b1a": "b1b", "b1b": "b1a", "b2": "b2r", "b3": "b3r", "b3r": "b3"}       # the second live counts of a static buffer set


def _id(case):
    return "-".join(str(v) for v in case)


@functools.lru_cache(maxsize=None)
def _cut_levels(layout, k, pattern):
    return [M.cut_level(counts, k, pattern, N_CLS, _seed(layout, k, pattern, li)) for li, counts in enumerate(_layouts(k)[layout])]


def _level_coords(lv):
    n = len(lv["scene"])
    return np.concatenate((lv["scene"][:, None], M.site(np.arange(n), TS)), axis=1)


def _eager_level(lv, n_reg, device):
    """one level of head outputs on the device, exact size"""
    from cnrma_amd import sparse as S
    pts, box = M.identity_rows(len(lv["scene"]), n_reg)
    cs = S.CoordSet(_dev(_level_coords(lv).astype(np.int32), device), TS, n_batch=len(lv["counts"]))
    cs.scene_major = True
    return dict(cen=_dev(lv["cen"], device), box=_dev(box, device), cls=_dev(lv["cls"], device), pts=_dev(pts, device), cs=cs)


def _check_rows(bx, sc, ids, d, lv, yaw, what):
    """the rows (bx, sc) a path returned for one scene on one level are the rows `ids`, in that order"""
    from cnrma_amd import sparse as S
    assert bx.shape[0] == sc.shape[0] == len(ids), (what, bx.shape, sc.shape, len(ids))
    if len(ids) == 0:
        return
    got = bx[:, 0].cpu().numpy()
    bad = np.nonzero(got != ids)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(ids)} rows differ, first at slot {bad[0]}: row {got[bad[0]]}, expected {ids[bad[0]]}"
    b2, s2 = S.select_decode(_dev(ids, bx.device), d["cls"], d["cen"], d["box"], d["pts"], yaw)
    assert torch.equal(bx.contiguous().view(torch.int32), b2.view(torch.int32)), what
    assert torch.equal(sc.contiguous().view(torch.int32), s2.view(torch.int32)), what
    exp = M.class_scores64(lv["cls"][ids], lv["cen"][ids])
    assert np.abs(sc.cpu().numpy().astype(np.float64) - exp).max() <= 1e-6, what
    pts, box = M.identity_rows(len(lv["scene"]), d["box"].shape[1])
    expb = SO.decode_boxes(torch.from_numpy(pts[ids]).double(), torch.from_numpy(box[ids]).double(), yaw).numpy()
    np.testing.assert_allclose(bx.cpu().numpy(), expb, rtol=1e-5, atol=1e-5)


def _expected_cut(levels, nms_pre):
    """[level][scene] -> row ids"""
    return [M.cut_rows(lv["scene"], lv["score"], nms_pre, len(lv["counts"])) for lv in levels]


def _check_per_scene(out, levels, devs, nms_pre, yaw, what):
    """out: [(bboxes, scores)] per scene, the levels concatenated (what the eager paths return)"""
    exp = _expected_cut(levels, nms_pre)
    assert len(out) == len(levels[0]["counts"])
    for b, (bx, sc) in enumerate(out):
        assert bx.shape[0] == sum(len(e[b]) for e in exp), (what, b, bx.shape)
        r0 = 0
        for li, (lv, d) in enumerate(zip(levels, devs)):
            n = len(exp[li][b])
            _check_rows(bx[r0:r0 + n], sc[r0:r0 + n], exp[li][b], d, lv, yaw, f"{what}, scene {b}, level {li}")
            r0 += n


def _single(head, devs, levels):
    """_get_bboxes_single through get_bboxes: every scene's slice of every level as the decomposed outputs"""
    per = {k: [] for k in ("cen", "box", "cls", "pts")}
    for lv, d in zip(levels, devs):
        off = np.concatenate(([0], np.cumsum(lv["counts"])))
        for k in per:
            per[k].append([d[k][off[b]:off[b + 1]] for b in range(len(lv["counts"]))])
    return head.get_bboxes(per["cen"], per["box"], per["cls"], per["pts"], None, None)


def _fused(head, devs, B):
    return head.get_bboxes_fused(*[[[d[k]] for d in devs] for k in ("cen", "box", "cls", "pts", "cs")], B)


@pytest.mark.parametrize("n_reg,yaw", MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", CUT_CASES, ids=_id)
def test_cut_eager_one_scene_at_a_time(device, case, n_reg, yaw):
    layout, k, pattern, nms_pre = case
    levels = _cut_levels(layout, k, pattern)
    devs = [_eager_level(lv, n_reg, device) for lv in levels]
    out = _single(_cut_head(n_reg, yaw, nms_pre), devs, levels)
    _check_per_scene(out, levels, devs, nms_pre, yaw, "_get_bboxes_single")


@pytest.mark.parametrize("n_reg,yaw", MODES, ids=lambda v: str(v))
@pytest.mark.parametrize("case", CUT_CASES, ids=_id)
def test_cut_eager_fused(device, case, n_reg, yaw):
    """one scene: the branch of _get_bboxes_single; several scenes: a scene at or below nms_pre rows keeps them in row order"""
    layout, k, pattern, nms_pre = case
    levels = _cut_levels(layout, k, pattern)
    devs = [_eager_level(lv, n_reg, device) for lv in levels]
    out = _fused(_cut_head(n_reg, yaw, nms_pre), devs, len(levels[0]["counts"]))
    _check_per_scene(out, levels, devs, nms_pre, yaw, "get_bboxes_fused")


# ---- the static forms ------------------------------------------------------------------------------------------------------
class _StaticLevel:
    """one level's head outputs in capacity buffers: rows >= the live count are poison"""

    def __init__(self, lv, cap, n_reg, poison, device):
        n = len(lv["scene"])
        pts, box = M.identity_rows(n, n_reg)
        self.cap, self.n_reg, self.poison, self.B = cap, n_reg, poison, len(lv["counts"])
        x = capacity_tensor(_level_coords(lv), lv["cen"], TS, device, cap=cap, value=poison, n_batch=self.B)
        self.cs, self.cen = x.cs, x.F
        self.C, self.n_dev = x.cs.C, x.cs.n_dev
        self.cls, self.box, self.pts = (poison_rows(a, cap, device, poison) for a in (lv["cls"], box, pts))
        self.lv = lv

    def refill(self, lv):
        """other rows and another live count in the same buffers, as a replay finds them"""
        from cnrma_amd import sparse as S
        n = len(lv["scene"])
        assert n <= self.cap and len(lv["counts"]) == self.B
        pts, box = M.identity_rows(n, self.n_reg)
        for buf, a in ((self.cen, lv["cen"]), (self.cls, lv["cls"]), (self.box, box), (self.pts, pts)):
            buf.fill_(self.poison)
            buf[:n] = _dev(a, buf.device)
        self.C.copy_(_dev(poison_coords(_level_coords(lv), self.cap, TS).astype(np.int32), self.C.device))
        self.n_dev.fill_(n)
        self.cs = S.CoordSet(self.C, TS, n_batch=self.B, n=self.cap, n_dev=self.n_dev)     # a trace derives its own caches
        assert self.cs.C.data_ptr() == self.C.data_ptr()
        self.lv = lv

    @property
    def d(self):
        return dict(cen=self.cen, box=self.box, cls=self.cls, pts=self.pts, cs=self.cs)


def _static_args(sl):
    return [[[getattr(s, k)] for s in sl] for k in ("cen", "box", "cls", "pts", "cs")]


def _second_count(n, k, flag):
    """another live count for which the plan flag of a level with n rows still holds (None: the other side of the cut)"""
    above = n > k
    if flag is None:
        return k - 1 if above else k + 1
    if above:
        return k + 1 if n > k + 1 else 2 * k + 3
    return k if n < k else k - 1


def _check_static_single(out, sl, flags, nms_pre, yaw, what):
    bx, sc, valid, sizes = out
    valid = valid.cpu().tolist()
    assert bx.shape[0] == sc.shape[0] == sum(sizes) and len(valid) == len(sl)
    r0 = 0
    for li, (s, flag) in enumerate(zip(sl, flags)):
        lv, n = s.lv, len(s.lv["scene"])
        topk = bool(flag) or (flag is None and s.cap > nms_pre > 0)
        assert sizes[li] == (nms_pre if topk else s.cap), (what, li, sizes)
        ids = M.cut_rows(lv["scene"], lv["score"], nms_pre, 1)[0]
        if topk and n <= nms_pre:                           # the documented deviation of the None form: all rows, best first
            ids = M.ranked(np.arange(n), lv["score"])
        assert valid[li] == len(ids), (what, li, valid, len(ids))
        _check_rows(bx[r0:r0 + len(ids)], sc[r0:r0 + len(ids)], ids, s.d, lv, yaw, f"{what}, level {li}")
        r0 += sizes[li]


@pytest.mark.parametrize("cap_mode", CAPS)
@pytest.mark.parametrize("poison", POISONS, ids=["3e38", "nan"])
@pytest.mark.parametrize("calibrated", [True, False], ids=["flags_exact", "flags_none"])
@pytest.mark.parametrize("case", B1_CASES, ids=_id)
def test_cut_static_one_scene(device, case, calibrated, poison, cap_mode):
    """get_bboxes_static under the flags a calibration on these counts records, and under None at every level (calibration
    scenes that disagreed: the top-k form, which below nms_pre rows gives all live rows best first and valid = their number).
    Then other rows with other live counts in the same buffers under the same plan."""
    layout, k, pattern, nms_pre = case
    n_reg, yaw = MODES[_seed(case) % 3]
    first = _cut_levels(layout, k, pattern)
    flags = [(len(lv["scene"]) > nms_pre > 0) if calibrated else None for lv in first]
    second = [M.cut_level((_second_count(len(lv["scene"]), k, f),), k, pattern, N_CLS, _seed(case, li, "second"))
              for li, (lv, f) in enumerate(zip(first, flags))]
    sl = [_StaticLevel(a, _capacity(max(len(a["scene"]), len(b["scene"])), cap_mode), n_reg, poison, device) for a, b in zip(first, second)]
    head, plan = _cut_head(n_reg, yaw, nms_pre), _plan(flags)
    for run, levels in enumerate((first, second)):
        if run:
            for s, lv in zip(sl, levels):
                s.refill(lv)
        out, status = _static(plan, device, lambda: head.get_bboxes_static(*_static_args(sl)))
        assert status == 0, (run, status)
        _check_static_single(out, sl, flags, nms_pre, yaw, f"get_bboxes_static run {run}")


@pytest.mark.parametrize("n,flag", [(64, True), (63, True), (0, True), (65, False), (131, False)])
def test_cut_static_one_scene_reports_a_broken_premise(device, n, flag):
    """flag True with a level at nms_pre rows or fewer, flag False with a level above nms_pre: the status word is not 0 (the
    three other levels keep their premise)"""
    k = 64
    counts = [n, 2 * k + 3, k, k + 1]
    flags = [flag, True, False, True]
    levels = [M.cut_level((c,), k, "plain", N_CLS, _seed("premise", c, li)) for li, c in enumerate(counts)]
    sl = [_StaticLevel(lv, max(c, k + 1) + 37, 6, 3e38, device) for lv, c in zip(levels, counts)]
    head = _cut_head(6, "fcaf3d", k)
    _, status = _static(_plan(flags), device, lambda: head.get_bboxes_static(*_static_args(sl)))
    assert status != 0
    ok = list(counts)
    ok[0] = k + 1 if flag else k
    sl[0].refill(M.cut_level((ok[0],), k, "plain", N_CLS, _seed("premise ok", n)))
    out, status = _static(_plan(flags), device, lambda: head.get_bboxes_static(*_static_args(sl)))
    assert status == 0
    _check_static_single(out, sl, flags, k, "fcaf3d", "get_bboxes_static")


def _check_static_multi(out, sl, nms_pre, yaw, what):
    bx, sc, valid, sizes = out
    B = sl[0].B
    valid = valid.cpu().numpy()
    assert bx.shape[:2] == sc.shape[:2] == (B, sum(sizes)) and valid.shape == (B, len(sl))
    r0 = 0
    for li, s in enumerate(sl):
        assert sizes[li] == (min(nms_pre, s.cap) if nms_pre > 0 else s.cap), (what, li, sizes)
        exp = M.cut_rows(s.lv["scene"], s.lv["score"], nms_pre, B)
        for b in range(B):
            n = len(exp[b])
            assert valid[b, li] == n, (what, b, li, valid[b, li], n)
            _check_rows(bx[b, r0:r0 + n], sc[b, r0:r0 + n], exp[b], s.d, s.lv, yaw, f"{what}, scene {b}, level {li}")
        r0 += sizes[li]


@pytest.mark.parametrize("cap_mode", CAPS)
@pytest.mark.parametrize("poison", POISONS, ids=["3e38", "nan"])
@pytest.mark.parametrize("case", CUT_CASES, ids=_id)
def test_cut_static_several_scenes(device, case, poison, cap_mode):
    """get_bboxes_static_multi (the benchmark's path), then the same buffers with the scenes in the other order (one scene:
    with the other layout's counts)"""
    layout, k, pattern, nms_pre = case
    n_reg, yaw = MODES[_seed(case) % 3]
    first, second = _cut_levels(layout, k, pattern), _cut_levels(OTHER[layout], k, pattern)
    B = len(first[0]["counts"])
    sl = [_StaticLevel(a, _capacity(max(len(a["scene"]), len(b["scene"])), cap_mode), n_reg, poison, device) for a, b in zip(first, second)]
    head, plan = _cut_head(n_reg, yaw, nms_pre), _plan([True, False, None, True])       # the flags are consumed, not used
    for run, levels in enumerate((first, second)):
        if run:
            for s, lv in zip(sl, levels):
                s.refill(lv)
        out, status = _static(plan, device, lambda: head.get_bboxes_static_multi(*_static_args(sl), B))
        assert status == 0
        _check_static_multi(out, sl, nms_pre, yaw, f"get_bboxes_static_multi run {run}")


@pytest.mark.parametrize("case", [("b1a", 64, "straddle5", 64), ("b1b", 64, "plain", 64), ("b3", 64, "zeros", 64), ("b2", 64, "equal", 0)],
                         ids=_id)
def test_cut_paths_agree(device, case):
    """the same input through every path that takes it: the same rows in the same order, bit for bit (one scene: all four
    paths; several: the three that take several, each scene as that scene alone through _get_bboxes_single)"""
    layout, k, pattern, nms_pre = case
    n_reg, yaw = 8, "fcaf3d"
    levels = _cut_levels(layout, k, pattern)
    B = len(levels[0]["counts"])
    devs = [_eager_level(lv, n_reg, device) for lv in levels]
    head = _cut_head(n_reg, yaw, nms_pre)
    single = _single(head, devs, levels)
    fused = _fused(head, devs, B)
    sl = [_StaticLevel(lv, len(lv["scene"]) + 37, n_reg, float("nan"), device) for lv in levels]
    (mb, ms, mvalid, msizes), status = _static(_plan([None] * 4), device, lambda: head.get_bboxes_static_multi(*_static_args(sl), B))
    assert status == 0
    mvalid = mvalid.cpu().numpy()
    multi = []
    for b in range(B):
        keep = np.concatenate([np.arange(v) + sum(msizes[:li]) for li, v in enumerate(mvalid[b])]).astype(np.int64)
        multi.append((mb[b][_dev(keep, device)], ms[b][_dev(keep, device)]))
    paths = [single, fused, multi]
    if B == 1:
        flags = [len(lv["scene"]) > nms_pre > 0 for lv in levels]
        (sb, ss, svalid, ssizes), status = _static(_plan(flags), device, lambda: head.get_bboxes_static(*_static_args(sl)))
        assert status == 0
        keep = np.concatenate([np.arange(v) + sum(ssizes[:li]) for li, v in enumerate(svalid.cpu().tolist())]).astype(np.int64)
        paths.append([(sb[_dev(keep, device)], ss[_dev(keep, device)])])
    for other in paths[1:]:
        for (b0, s0), (b1, s1) in zip(single, other):
            assert b0.shape == b1.shape and torch.equal(b0.view(torch.int32), b1.contiguous().view(torch.int32))
            assert torch.equal(s0.view(torch.int32), s1.contiguous().view(torch.int32))


# =====================================================================================================================
# the pruning
# =====================================================================================================================
def _mixes(T):
    return {"n1": (1,), "below": (T - 1,), "at": (T,), "above": (T + 1,), "far": (2 * T + 3,),
            "b2": (T + 1, T), "b2e": (T + 1, 0), "b3": (2 * T + 3, 0, T - 1), "b3r": (T - 1, 0, 2 * T + 3)}


PRUNE_OTHER = {"n1": "above", "below": "above", "at": "far", "above": "at", "far": "below", "b2": "b3x", "b2e": "b2", "b3": "b3r", "b3r": "b3"}
# (mix, T, pattern, off_site)
PRUNE_CASES = [(mix, T, "plain", False) for T in (64, 1000, 1500) for mix in ("n1", "below", "at", "above", "far", "b2", "b2e", "b3", "b3r")] \
    + [(mix, T, pat, False) for T in (64, 1000) for mix in ("far", "b3") for pat in M.PATTERNS[1:]] \
    + [(mix, 64, pat, True) for mix in ("far", "b2", "b3") for pat in ("plain", "straddle5")]


@functools.lru_cache(maxsize=None)
def _prune_case(counts, T, pattern, off_site):
    """the inputs, the float64 interpolation of the score field at the queries (the oracle's) and the rows the model keeps"""
    lv = M.prune_level(counts, T, pattern, TS, _seed(counts, T, pattern, off_site), off_site)
    lv["interp"] = SO.interpolate(lv["score_coords"], lv["score"], 2 * TS, lv["coords"]).reshape(-1)
    lv["kept"] = M.prune_rows(lv["scene"], lv["interp"], T, len(counts))
    return lv


def _check_pruned(out, lv, T, static, cap, what):
    rows, B = lv["kept"], len(lv["counts"])
    if static:
        assert out.cs.n == min(B * T, cap) and out.F.shape[0] == out.cs.n, (what, out.cs.n, B * T, cap)
        live = int(out.cs.n_dev.cpu()[0])
    else:
        assert out.cs.n_dev is None
        live = out.cs.n
        assert list(out.cs.batch_counts()) == [min(c, T) for c in lv["counts"]], what
    assert live == len(rows), (what, live, len(rows))
    assert out.cs.n_batch == B and out.cs.stride == TS
    got = out.F[:live, 0].cpu().numpy()
    bad = np.nonzero(got != rows)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {live} kept rows differ, first at slot {bad[0]}: row {got[bad[0]]}, expected {rows[bad[0]]}"
    assert np.array_equal(out.C[:live].cpu().numpy(), lv["coords"][rows]), what
    assert np.array_equal(out.F[:live].cpu().numpy(), lv["feats"][rows]), what


@pytest.mark.parametrize("case", PRUNE_CASES, ids=_id)
def test_prune_eager(device, case):
    """one scene: one radix select; several scenes: one per scene that is above the threshold"""
    mix, T, pattern, off_site = case
    lv = _prune_case(_mixes(T)[mix], T, pattern, off_site)
    B = len(lv["counts"])
    x = capacity_tensor(lv["coords"], lv["feats"], TS, device, n_batch=B)
    scores = capacity_tensor(lv["score_coords"], lv["score"], 2 * TS, device, n_batch=B)
    out = _prune_head(T)._prune(x, scores)
    if all(c <= T for c in lv["counts"]):
        assert out is x
    _check_pruned(out, lv, T, False, None, "eager _prune")
    assert _prune_head(-1)._prune(x, scores) is x


def _prune_buffers(lv, cap, score_cap, poison, device, n_batch=None):
    B = len(lv["counts"]) if n_batch is None else n_batch
    return (capacity_tensor(lv["coords"], lv["feats"], TS, device, cap=cap, value=poison, n_batch=B),
            capacity_tensor(lv["score_coords"], lv["score"], 2 * TS, device, cap=score_cap, value=poison, n_batch=B))


def _refill(t, coords, feats, ts, poison):
    """other rows and another live count in a capacity tensor's buffers -> a fresh SparseTensor over them"""
    from cnrma_amd import sparse as S
    cap, n = t.cs.n, len(coords)
    assert n < cap
    t.F.fill_(poison)
    t.F[:n] = _dev(np.asarray(feats, dtype=np.float32), t.F.device)
    t.cs.C.copy_(_dev(poison_coords(coords, cap, ts).astype(np.int32), t.F.device))
    t.cs.n_dev.fill_(n)
    return S.SparseTensor(t.F, S.CoordSet(t.cs.C, ts, n_batch=t.cs.n_batch, n=cap, n_dev=t.cs.n_dev))


@pytest.mark.parametrize("cap_mode", CAPS)
@pytest.mark.parametrize("poison", POISONS, ids=["3e38", "nan"])
@pytest.mark.parametrize("flag", [False, None], ids=["flag_false", "flag_none"])
@pytest.mark.parametrize("case", PRUNE_CASES, ids=_id)
def test_prune_static(device, case, flag, poison, cap_mode):
    """the static trace with one scene (one select under the live word) and with several (one select per scene), then other
    rows with other live counts in the same buffers"""
    mix, T, pattern, off_site = case
    mixes = _mixes(T)
    mixes["b3x"] = (T, T + 1)
    first = _prune_case(mixes[mix], T, pattern, off_site)
    second = _prune_case(mixes[PRUNE_OTHER[mix]], T, pattern, off_site)
    cap = _capacity(max(len(first["scene"]), len(second["scene"])), cap_mode)
    score_cap = _capacity(max(len(first["score"]), len(second["score"])), cap_mode)
    x, scores = _prune_buffers(first, cap, score_cap, poison, device)
    head, plan = _prune_head(T), _plan([flag])
    for run, lv in enumerate((first, second)):
        if run:
            x = _refill(x, lv["coords"], lv["feats"], TS, poison)
            scores = _refill(scores, lv["score_coords"], lv["score"], 2 * TS, poison)
        out, status = _static(plan, device, lambda: head._prune(x, scores))
        assert status == 0, (run, status)
        _check_pruned(out, lv, T, True, cap, f"static _prune run {run}")


@pytest.mark.parametrize("T,pattern", [(64, "straddle5"), (1000, "plain"), (1500, "zeros")])
def test_prune_forms_agree(device, T, pattern):
    """the same rows of one scene through all four forms -- declared as one scene, and as the first of two scenes of which the
    second is empty, eager and static --: the same kept rows, coordinates and features bit for bit"""
    lv = _prune_case((2 * T + 3,), T, pattern, False)
    n, rows, head = len(lv["scene"]), lv["kept"], _prune_head(T)
    assert len(rows) == T
    outs = []
    for n_batch in (1, 2):
        x = capacity_tensor(lv["coords"], lv["feats"], TS, device, n_batch=n_batch)
        scores = capacity_tensor(lv["score_coords"], lv["score"], 2 * TS, device, n_batch=n_batch)
        out = head._prune(x, scores)
        assert out.cs.n == T and list(out.cs.batch_counts()) == [T, 0][:n_batch]
        outs.append((out.C, out.F))
        x, scores = _prune_buffers(lv, n + 37, n + 37, float("nan"), device, n_batch)
        out, status = _static(_plan([False]), device, lambda: head._prune(x, scores))
        assert status == 0 and out.cs.n == min(n_batch * T, n + 37) and int(out.cs.n_dev.cpu()[0]) == T
        outs.append((out.C[:T], out.F[:T]))
    for C, F in outs:
        assert np.array_equal(C.cpu().numpy(), lv["coords"][rows]) and np.array_equal(F.cpu().numpy(), lv["feats"][rows])


@pytest.mark.parametrize("mix,bad", [("at", "above"), ("b3", "b3bad"), ("b2ok", "b2")])
def test_prune_static_skip(device, mix, bad):
    """plan flag True (no calibration scene needed pruning): the input comes back as it is; the status word is 0 while every
    scene has at most pts_threshold rows and not 0 when one has a row more.  pts_threshold < 0 switches the step off."""
    T = 64
    mixes = _mixes(T)
    mixes["b3"], mixes["b3bad"], mixes["b2ok"] = (T, 0, T - 1), (T - 1, 0, T + 1), (T - 1, T)
    good, worse = _prune_case(mixes[mix], T, "plain", False), _prune_case(mixes[bad], T, "plain", False)
    cap = max(len(good["scene"]), len(worse["scene"])) + 37
    x, scores = _prune_buffers(good, cap, cap, 3e38, device)
    head, plan = _prune_head(T), _plan([True])
    out, status = _static(plan, device, lambda: head._prune(x, scores))
    assert out is x and status == 0
    x = _refill(x, worse["coords"], worse["feats"], TS, 3e38)
    out, status = _static(plan, device, lambda: head._prune(x, scores))
    assert out is x and status != 0
    out, status = _static(_plan([]), device, lambda: _prune_head(-1)._prune(x, scores))
    assert out is x and status == 0
