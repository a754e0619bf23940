"""The kernels of csrc/targets.hip against the reference and at the sizes where their loops turn over.

A. sparse.assign_targets and FCAF3DHead(device_targets=True).loss against tests/golden/fcaf3d_assign.npz: the reference's own
   assigner and loss composition on boxes with yaw 0 (make_golden.py run_assign / run_head_loss), (cos 0, sin 0) = (1, 0)
   uploaded.  The head's three losses under the rule of tests/test_target_losses_gpu.py (_within): the device path's error
   against the recorded float64 values may be at most twice that of the float32 torch modules, plus one float32 ulp.

B. The yardstick is FCAF3DAssigner.assign of this repository in float32 on the CPU with the pinned square root -- which
   tests/test_targets_reference_cpu.py anchors to the reference -- compared bit for bit by the rules of _check in
   tests/test_targets_gpu.py, rotated boxes included: the second round of the single-workgroup scan (more than 1024 row blocks),
   more boxes than a workgroup has threads (m_cap = 304 and the ceiling 1024), topk = 1, topk + 1 > n, limit = 0 and 1, an empty
   first / last level and a single level, int32 ground-truth labels through the C ABI.  The focal kernel past its 4096-block
   cap (grid-stride loop), with one class, and with gamma = 1.5, 0, 1; the positive-row kernel and its column sums over
   p_cap = 1024 x 18 rows with 0, 1, 63, 64, 65 and p_cap live ones -- these against the float64 evaluation of the torch
   modules under _within.  Every result is computed twice and must be identical; before each comparison the yardstick is
   asserted to show the situation the case is about.  Labels of the B scenes are the box indices, so a label names its box."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cnrma_amd import _lib
from cnrma_amd import sparse as S
from projects.mvsdetection.core.boxes import GTBoxes
from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead, _SigmoidFocalLoss
from targets_fixture import (ASSIGN_SCENES, PinnedSqrtAssigner, assign_on_cpu, assign_scene, load_targets_fixture, loss_scene)
from test_target_losses_gpu import _positive_reference, _within
from test_targets_gpu import _box, _scene

pytestmark = pytest.mark.gpu
LIMIT, TOPK = 27, 18
ROWS_PER_BLOCK, SCAN_WIDTH = 256, 1024                      # TGT_BLOCK rows per row block; blocks per round of tgt_scan_kernel


def _identical(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _check(exp, gt, got, n_boxes, topk):
    """exp: labels [n], pos_box_target [P, 7], pos_ctr [P] of the rows with label >= 0 in ascending order"""
    labels, pos_row, pos_box, pos_ctr, n_pos = got
    n_pos = int(n_pos)
    lab = exp["labels"].long()
    assert labels.dtype == torch.int32 and torch.equal(labels.long(), lab)
    pos = torch.nonzero(lab >= 0).view(-1)
    assert n_pos == len(pos) <= n_boxes * topk
    assert torch.equal(pos_row[:n_pos].long(), pos)                                       # ascending row order
    jb = pos_box[:n_pos].long()
    assert torch.equal(gt.boxes.cpu()[jb].view(torch.int32), exp["pos_box_target"].view(torch.int32))      # box target, bit for bit
    assert torch.equal(gt.labels.cpu()[jb].long(), lab[pos])                              # the box (its label is its own)
    assert torch.equal(pos_ctr[:n_pos].view(torch.int32), exp["pos_ctr"].view(torch.int32))                # centerness target, bit for bit
    assert not pos_row[n_pos:].any() and not pos_box[n_pos:].any() and not pos_ctr[n_pos:].view(torch.int32).any()
    assert pos_row.shape[0] == gt.boxes.shape[0] * topk
    return pos, jb


# ---- A: against the reference's fixture -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return load_targets_fixture()


@pytest.mark.parametrize("name", ASSIGN_SCENES)
def test_assign_targets_equals_the_reference(device, fixture, name):
    sc = assign_scene(fixture, name)
    limit, topk = (int(v) for v in sc["limit_topk"])
    assert (sc["boxes"][:, 6] == 0).all() and (sc["labels"] >= 0).any()
    gt = S.DeviceGT.from_boxes(GTBoxes(torch.from_numpy(sc["boxes"])), torch.from_numpy(sc["gt_labels"]).long(), device)
    cs = torch.tensor([1.0, 0.0], device=device).repeat(gt.boxes.shape[0], 1)
    run = lambda: [o.cpu() for o in S.assign_targets(torch.cat([torch.from_numpy(p) for p in sc["levels"]]).to(device),
                                                     [len(p) for p in sc["levels"]], gt, limit, topk, cs=cs)]
    got = run()
    exp = dict(labels=torch.from_numpy(sc["labels"]), pos_box_target=torch.from_numpy(sc["pos_box_target"]),
               pos_ctr=torch.from_numpy(sc["pos_centerness"]))
    _check(exp, gt, got, len(sc["boxes"]), topk)
    _identical(got, run())


def _loss_of_two_scenes(head, scenes, device, dtype=torch.float32):
    per_level = lambda key: [[torch.from_numpy(sc[key][l]).to(device=device, dtype=dtype).requires_grad_(True) for sc in scenes]
                             for l in range(4)]
    loss = head.loss(per_level("centerness"), per_level("bbox_pred"), per_level("cls_score"),
                     [[torch.from_numpy(sc["points"][l]).to(device) for sc in scenes] for l in range(4)],
                     [GTBoxes(torch.from_numpy(sc["boxes"])).to(device) for sc in scenes],
                     [torch.from_numpy(sc["gt_labels"]).long().to(device) for sc in scenes])
    return [loss[k].detach().cpu() for k in ("loss_centerness", "loss_bbox", "loss_cls")]


def test_device_head_loss_equals_the_reference(device, fixture):
    """two scenes in one call, the second without a positive row: the mean over scenes of the three losses"""
    scenes = [loss_scene(fixture, s) for s in range(2)]
    assert (scenes[0]["handed"]["cls_labels"] >= 0).any() and not (scenes[1]["handed"]["cls_labels"] >= 0).any()
    make = lambda on: FCAF3DHead(n_classes=18, in_channels=(8, 8, 8, 8), out_channels=8, n_reg_outs=6, voxel_size=.01,
                                 pts_threshold=100000, assigner=dict(type="FCAF3DAssigner", limit=LIMIT, topk=TOPK, n_scales=4),
                                 device_targets=on)
    cpu_head = make(False)
    cpu_head.assigner = PinnedSqrtAssigner(cpu_head.assigner)
    t32 = _loss_of_two_scenes(cpu_head, scenes, torch.device("cpu"))
    got = _loss_of_two_scenes(make(True), scenes, device)
    for i, key in enumerate(("loss_centerness", "loss_bbox", "loss_cls")):
        assert got[i].dtype == torch.float32
        _within(f"{key} against the reference", got[i], torch.tensor(float(fixture[f"loss.{key}"]), dtype=torch.float64), t32[i])
    _identical(got, _loss_of_two_scenes(make(True), scenes, device))


# ---- B: the assignment kernels --------------------------------------------------------------------------------------------------------
def _uniform_levels(rng, sizes):
    return [torch.from_numpy(rng.uniform(0, 2, (n, 3)).astype(np.float32)) for n in sizes]


def _random_boxes(rng, m, lo, hi, big_every=None):
    """m boxes with sides in [lo, hi) -- every big_every-th with sides in [1.1, 1.5): enough points on a coarser level -- and
    every second one rotated"""
    return [_box(*rng.uniform(.2, 1.8, 3), *(rng.uniform(1.1, 1.5, 3) if big_every and i % big_every == big_every - 1 else rng.uniform(lo, hi, 3)),
                 rng.uniform(-3.5, 3.5) if i % 2 else 0.0) for i in range(m)]


@functools.lru_cache(maxsize=None)
def _edge_scene(name):
    """(levels, box rows) -- built once, never modified; the label of a box is its index"""
    if name == "scan":
        # level 0: 262 400 rows = 1025 row blocks, in ascending x: block 1024, the first of the second scan round, is its last.
        # Box 0 (small, at high x) and box 2 (small, rotated, at low x) win rows of level 0 inside the first round; box 1 has
        # >= 27 points on levels 0 and 1 but not on level 2, so its rows lie on level 1, in the second round.
        rng = np.random.RandomState(5)
        l0 = rng.uniform(0, 2, (262400, 3)).astype(np.float32)
        l0 = torch.from_numpy(l0[np.argsort(l0[:, 0], kind="stable")])
        return [l0] + _uniform_levels(rng, (300, 40)), [_box(1.6, 1.0, 1.0, .3, .3, .3), _box(1.0, 1.0, 1.0, 1.3, 1.3, 1.3),
                                                          _box(.3, .5, .5, .25, .3, .2, .7)]
    if name == "boxes300":
        rng = np.random.RandomState(6)
        return _uniform_levels(rng, (2401, 517, 99)), _random_boxes(rng, 300, .15, .6, 16)
    if name == "boxes1024":
        rng = np.random.RandomState(7)
        return _uniform_levels(rng, (1000, 150, 50)), _random_boxes(rng, 1024, .15, .6, 16)
    if name == "awkward":
        levels, rows, _ = _scene("awkward")
        return levels, rows
    rng = np.random.RandomState(8)
    rows = _random_boxes(rng, 4, .5, 1.2) + [_box(1.0, 1.0, 1.0, 1.8, 1.8, 1.8, .4)]      # the last one: >= 27 of 60 points
    if name == "first_level_empty":
        return _uniform_levels(rng, (0, 500, 60)), rows
    if name == "last_level_empty":
        return _uniform_levels(rng, (500, 60, 0)), rows
    if name == "one_level":
        return _uniform_levels(rng, (500,)), rows
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _yardstick(name, limit=LIMIT, topk=TOPK):
    levels, rows = _edge_scene(name)
    gt = GTBoxes(torch.tensor(rows, dtype=torch.float32))
    ctr, box_t, lab = assign_on_cpu(levels, gt, torch.arange(len(rows)), limit, topk)
    pos = torch.nonzero(lab >= 0).view(-1)
    ang = -gt.tensor[:, 6]
    return dict(labels=lab, pos=pos, pos_box_target=box_t[pos], pos_ctr=ctr[pos], cs=torch.stack((torch.cos(ang), torch.sin(ang)), 1))


def _run(name, device, limit=LIMIT, topk=TOPK, m_cap=None):
    levels, rows = _edge_scene(name)
    gt = S.DeviceGT.from_boxes(GTBoxes(torch.tensor(rows, dtype=torch.float32)), torch.arange(len(rows)), device, m_cap=m_cap)
    cs = torch.zeros((gt.boxes.shape[0], 2))
    cs[:len(rows)] = _yardstick(name, limit, topk)["cs"]
    cs, points = cs.to(device), torch.cat(levels).to(device)
    run = lambda: [o.cpu() for o in S.assign_targets(points, [len(p) for p in levels], gt, limit, topk, cs=cs)]
    got = run()
    _identical(got, run())
    return gt, got


def _row_levels(name, rows):
    return np.searchsorted(np.cumsum([len(p) for p in _edge_scene(name)[0]]), rows.numpy(), side="right")


def test_second_round_of_the_scan(device):
    levels, rows = _edge_scene("scan")
    ref = _yardstick("scan")
    n_blocks = sum(-(-len(p) // ROWS_PER_BLOCK) for p in levels)
    assert SCAN_WIDTH < n_blocks < 2 * SCAN_WIDTH                                      # two rounds
    first_round = ref["pos"] < SCAN_WIDTH * ROWS_PER_BLOCK
    lab, lv = ref["labels"][ref["pos"]], _row_levels("scan", ref["pos"])
    assert first_round.any() and (~first_round).any()                                 # positives on both sides of block 1024
    assert set(lab[first_round].tolist()) == {0, 2} and set(lv[first_round.numpy()].tolist()) == {0}
    assert set(lab[~first_round].tolist()) == {1} and set(lv[~first_round.numpy()].tolist()) == {1}
    assert int(ref["pos"][lab == 0].min()) > len(levels[0]) // 2                      # box 0: late rows of level 0
    gt, got = _run("scan", device)
    _check(ref, gt, got, len(rows), TOPK)


@pytest.mark.parametrize("name, m, m_cap", [("boxes300", 300, 304), ("boxes1024", 1024, 1024)])
def test_more_boxes_than_a_workgroup_has_threads(device, name, m, m_cap):
    ref = _yardstick(name)
    winners = set(ref["labels"][ref["pos"]].tolist())
    # boxes past every multiple of the 256 threads win rows, and more than 256 boxes do; box targets of rotated boxes among them
    assert len(winners) > 256 and all(any(lo <= w < lo + 256 for w in winners) for lo in range(0, m, 256))
    assert max(winners) >= m - 8 and (ref["pos_box_target"][:, 6] != 0).any()
    assert len(set(_row_levels(name, ref["pos"]).tolist())) >= 2                      # more than one best level
    gt, got = _run(name, device, m_cap=m_cap)
    assert gt.boxes.shape[0] == m_cap and got[1].shape[0] == m_cap * TOPK
    _check(ref, gt, got, m, TOPK)


def test_more_boxes_than_the_ceiling_is_an_error(device):
    levels, _ = _edge_scene("one_level")
    gt = S.DeviceGT(torch.zeros((1040, 7), device=device), torch.zeros(1040, dtype=torch.int64, device=device),
                    torch.zeros(1, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="1024"):
        S.assign_targets(levels[0].to(device), [len(levels[0])], gt, LIMIT, TOPK)


@pytest.mark.parametrize("limit, topk", [(27, 1), (27, 4000), (0, 18), (1, 18), (1, 1)])
def test_k_and_best_level_edges(device, limit, topk):
    levels, rows = _edge_scene("awkward")
    n = sum(len(p) for p in levels)
    ref = _yardstick("awkward", limit, topk)
    per_box = np.bincount(ref["labels"][ref["pos"]].numpy(), minlength=len(rows))
    lv = _row_levels("awkward", ref["pos"])
    assert len(ref["pos"]) > 0
    if topk == 1:                                             # k = 2: the best row of a box, unless a smaller box takes it
        assert per_box.max() == 1 and per_box.sum() >= 3
    if topk + 1 > n:                                          # k = n: the k-th value is a non-candidate's -1, every candidate passes
        assert per_box.max() > TOPK
    if limit == 0:                                            # no level has fewer than 0 points: always the last level
        assert set(lv.tolist()) == {len(levels) - 1}
    if limit == 1:                                            # the last level that still holds a point of the box: several levels
        assert len(set(lv.tolist())) >= 2 and set(lv.tolist()) != set(_row_levels("awkward", _yardstick("awkward")["pos"]).tolist())
    gt, got = _run("awkward", device, limit, topk)
    _check(ref, gt, got, len(rows), topk)


@pytest.mark.parametrize("name, limit, levels_hit", [("first_level_empty", 27, ()), ("first_level_empty", 0, (2,)),
                                                     ("last_level_empty", 27, (0, 1)), ("one_level", 27, (0,))])
def test_empty_levels_and_a_single_level(device, name, limit, levels_hit):
    """an empty first level holds fewer than `limit` points of every box, so it is every box's best level and no row is positive
    (the reference's rule) -- unless limit = 0, where the last level is; an empty last level sends the large boxes to level 1"""
    levels, rows = _edge_scene(name)
    ref = _yardstick(name, limit)
    assert tuple(sorted(set(_row_levels(name, ref["pos"]).tolist()))) == levels_hit
    assert len(ref["pos"]) > 0 or name == "first_level_empty"
    gt, got = _run(name, device, limit)
    _check(ref, gt, got, len(rows), TOPK)


def test_int32_labels_through_the_c_abi(device):
    """label_is_i64 = 0: tgt_assign_kernel<int32_t>; the labels are large and distinct, so reading them as int64 shows"""
    levels, rows = _edge_scene("awkward")
    ref = _yardstick("awkward")
    assert len(set(ref["labels"][ref["pos"]].tolist())) >= 3
    gt64 = S.DeviceGT.from_boxes(GTBoxes(torch.tensor(rows, dtype=torch.float32)), torch.arange(len(rows)), device)
    m_cap, n = gt64.boxes.shape[0], sum(len(p) for p in levels)
    names = torch.full((m_cap,), -5, dtype=torch.int32)
    names[:len(rows)] = 70000 + 1001 * torch.arange(len(rows), dtype=torch.int32)
    labels32 = names.to(device)
    cs = torch.zeros((m_cap, 2))
    cs[:len(rows)] = ref["cs"]
    cs, points = cs.to(device), torch.cat(levels).to(device)
    volume = (gt64.boxes[:, 3] * gt64.boxes[:, 4] * gt64.boxes[:, 5]).contiguous()
    caps = (ctypes.c_int32 * len(levels))(*[len(p) for p in levels])
    ws = _lib.scratch("cnrma_fcaf3d_assign_workspace_bytes", n, len(levels), m_cap, device=device)
    assert ws.numel() > 0

    def run():
        out = [torch.full((n,), -9, dtype=torch.int32, device=device)] + \
              [torch.full((m_cap * TOPK,), -9, dtype=t, device=device) for t in (torch.int32, torch.int32, torch.float32)] + \
              [torch.full((1,), -9, dtype=torch.int32, device=device)]
        _lib.call("cnrma_fcaf3d_assign_f32", _lib.ptr(points), ctypes.addressof(caps), len(levels), None, _lib.ptr(gt64.boxes),
                  _lib.ptr(cs), _lib.ptr(volume), _lib.ptr(labels32), 0, m_cap, _lib.ptr(gt64.n_live), LIMIT, TOPK, _lib.ptr(ws),
                  ws.numel(), *[_lib.ptr(o) for o in out], _lib.stream())
        return [o.cpu() for o in out]

    got = run()
    exp = dict(ref, labels=torch.where(ref["labels"] >= 0, names.long()[ref["labels"].clamp(min=0)], ref["labels"]))
    _check(exp, S.DeviceGT(gt64.boxes, labels32, gt64.n_live), got, len(rows), TOPK)
    _identical(got, run())


# ---- B: the focal kernel ----------------------------------------------------------------------------------------------------------------
def _focal_case(caps, live, n_cls, seed):
    rng = np.random.RandomState(seed)
    n = sum(caps)
    x = (rng.randn(n, n_cls) * 4).astype(np.float32)
    x[rng.rand(n, n_cls) < 0.02] = 30.0
    x[rng.rand(n, n_cls) < 0.02] = -30.0
    labels = np.full(n, -1, dtype=np.int32)
    hit = rng.rand(n) < 0.2
    labels[hit] = rng.randint(0, n_cls, hit.sum())
    labels[3], labels[4] = n_cls, 0                                 # outside [0, n_cls): a background row; class 0
    x[4, 0] = 30.0
    keep = np.concatenate([np.arange(c) < l for c, l in zip(caps, live)])
    x[~keep] = np.nan                                               # dead rows hold anything
    labels[~keep] = 0
    return torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(keep)


def _focal_reference(x, labels, gamma, dtype):
    p = x.to(dtype).requires_grad_(True)
    loss = _SigmoidFocalLoss(gamma=gamma, alpha=0.25)(p, labels.long(), avg_factor=1.0)
    return loss.detach(), torch.autograd.grad(loss, p)[0]


@pytest.mark.parametrize("caps, live, n_cls, gamma", [
    ((58300, 40), (58211, 33), 18, 2.0),                            # 1 050 120 elements: past 4096 blocks of 256, the grid-stride loop
    ((300,), (300,), 1, 2.0), ((211, 89), (200, 89), 1, 2.0),       # one class: row == element
    ((300,), (291,), 18, 1.5), ((300,), (291,), 18, 0.0), ((300,), (291,), 18, 1.0)])
def test_focal_kernel_at_its_edges(device, caps, live, n_cls, gamma):
    x, labels, keep = _focal_case(caps, live, n_cls, seed=len(caps) + n_cls)
    assert (sum(caps) * n_cls > 4096 * 256) == (len(caps) == 2 and n_cls == 18)
    assert (~keep).any() or n_cls == 1
    assert ((labels[keep] >= 0) & (labels[keep] < n_cls)).any() and (labels[keep] < 0).any() and (x[keep].abs() == 30).any()
    exp, g_exp = _focal_reference(x[keep], labels[keep], gamma, torch.float64)
    t32, g_t32 = _focal_reference(x[keep], labels[keep], gamma, torch.float32)
    assert torch.isfinite(g_t32).all() and float(g_exp.abs().max()) > 1e-3
    live_d = torch.tensor(live, dtype=torch.int32, device=device)

    def run():
        xd = x.to(device).requires_grad_(True)
        out = S.focal_loss_sum(xd, labels.to(device), caps, live_d, gamma, 0.25)
        (g,) = torch.autograd.grad(out, xd)
        return out.detach().cpu(), g.cpu()

    out, g = run()
    _within(f"focal sum, gamma {gamma}", out, exp, t32)
    _within(f"focal gradient, element by element, gamma {gamma}", g[keep], g_exp, g_t32)
    assert not g[~keep].view(torch.int32).any()                     # zeros on dead rows, whatever they hold
    _identical((out, g), run())


# ---- B: the positive rows ---------------------------------------------------------------------------------------------------------------
M_CAP = 1024
P_CAP = M_CAP * TOPK


@functools.lru_cache(maxsize=None)
def _positive_inputs(rotated):
    """ground truth [1024, 7] and P_CAP rows of predictions around it; the first n_pos rows of it are one case"""
    rng = np.random.RandomState(40 + rotated)
    gt = np.zeros((M_CAP, 7), dtype=np.float32)
    gt[:, :3] = rng.randn(M_CAP, 3) * 0.6
    gt[:, 3:6] = 0.3 + rng.rand(M_CAP, 3) * 1.5
    if rotated:
        gt[:, 6] = rng.uniform(-np.pi, np.pi, M_CAP)
    pos_box = rng.randint(0, M_CAP, P_CAP).astype(np.int32)
    pos_box[:3] = (M_CAP - 1, 0, 256)
    pos_ctr = rng.rand(P_CAP).astype(np.float32)
    t = gt[pos_box]
    pred = np.zeros((P_CAP, 7 if rotated else 6), dtype=np.float32)
    pred[:, :3] = t[:, :3] + rng.randn(P_CAP, 3) * 0.25
    pred[:, 3:6] = t[:, 3:6] * rng.uniform(0.6, 1.5, (P_CAP, 3))
    if rotated:
        pred[:, 6] = t[:, 6] + rng.randn(P_CAP) * 0.5
    logit = (rng.randn(P_CAP) * 3).astype(np.float32)
    logit[:2] = (30.0, -30.0)
    return tuple(torch.from_numpy(a) for a in (gt, pos_box, pos_ctr, pred, logit))


@functools.lru_cache(maxsize=None)
def _positive_yardstick(rotated, n_pos):
    inp = _positive_inputs(rotated)
    return _positive_reference(*inp, n_pos, rotated, torch.float64), _positive_reference(*inp, n_pos, rotated, torch.float32)


@pytest.mark.parametrize("n_pos", [0, 1, 63, 64, 65, P_CAP])
@pytest.mark.parametrize("rotated", [False, True])
def test_positive_rows_in_many_blocks(device, rotated, n_pos):
    gt, pos_box, pos_ctr, pred, logit = (t.clone() for t in _positive_inputs(rotated))
    pos_box[n_pos:], pos_ctr[n_pos:] = 0, 0.0                      # what assign_targets leaves behind n_pos
    pred[n_pos:], logit[n_pos:] = float("nan"), float("nan")       # dead rows hold anything
    g = S.DeviceGT(gt.to(device), torch.zeros(M_CAP, dtype=torch.int64, device=device),
                   torch.full((1,), M_CAP, dtype=torch.int32, device=device))

    def run():
        x, b = logit.to(device).requires_grad_(True), pred.to(device).requires_grad_(True)
        sums = S.positive_loss_sums(x, b, g, pos_box.to(device), pos_ctr.to(device),
                                    torch.full((1,), n_pos, dtype=torch.int32, device=device), rotated)
        gx, gb = torch.autograd.grad(sums[0] + sums[1], (x, b))
        return sums.detach().cpu(), gx.cpu(), gb.cpu()

    sums, gx, gb = run()
    assert sums.shape == (3,) and gx.shape == (P_CAP,) and gb.shape == pred.shape
    assert not gx[n_pos:].view(torch.int32).any() and not gb[n_pos:].view(torch.int32).any()       # dead rows: zero gradients
    if n_pos == 0:
        assert not sums.view(torch.int32).any()
    else:
        exp, t32 = _positive_yardstick(rotated, n_pos)
        assert float(exp[0]) > 0 and float(exp[1]) > 0 and float(exp[4].abs().max()) > 1e-3
        assert not rotated or float(exp[4][:, 6].abs().max()) > 1e-3
        for i, what in enumerate(("centerness BCE sum", "IoU loss sum", "sum of centerness targets")):
            _within(f"{what}, {n_pos} rows", sums[i], exp[i], t32[i])
        _within(f"centerness gradient, {n_pos} rows", gx[:n_pos], exp[3], t32[3])
        _within(f"box gradient, {n_pos} rows", gb[:n_pos], exp[4], t32[4])
    _identical((sums, gx, gb), run())
