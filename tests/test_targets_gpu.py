"""FCAF3D target assignment on the device (cnrma_amd.sparse.assign_targets / cnrma_fcaf3d_assign_f32) against the yardstick:
FCAF3DAssigner.assign run on the CPU in fp32, with (cos, sin) of the same CPU call uploaded.  Labels are compared on all rows;
the positive rows' box, box target and centerness target bit for bit (the torch result holds NaN on background rows: those are
not compared).  limit = 27, topk = 18 throughout.

One primitive of the yardstick is pinned: torch.sqrt.  On the CPU torch hands a contiguous sqrt to a vector math library that
is accurate to within one ulp but not correctly rounded, and which values it misses depends on the tensor's size and on the
processor (measured: 32 of 5000 uniform values on one machine; 11 of the 90 centerness targets of the "awkward" scene below on
another, none of them on the first).  The kernel's contract is the IEEE square root, so the yardstick runs with torch.sqrt
replaced by a correctly rounded one (numpy's); every other operation is torch's own, and the comparison stays bit for bit."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from cnrma_amd import sparse as S
from projects.mvsdetection.core.boxes import GTBoxes
from projects.mvsdetection.models.fcaf3d_head import FCAF3DAssigner

pytestmark = pytest.mark.gpu
LIMIT, TOPK = 27, 18


def _cells(n, step):
    g = (torch.arange(n, dtype=torch.float32) + 0.5) * step
    return torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()


def _lattice(shapes=((12, .08), (6, .16), (3, .32), (2, .64))):
    return [_cells(n, s) for n, s in shapes]


def _box(cx, cy, cz, dx, dy, dz, yaw=0.0):
    """(x, y, z_bottom, dx, dy, dz, yaw) of the box with gravity centre (cx, cy, cz)"""
    return [cx, cy, cz - dz / 2, dx, dy, dz, yaw]


def _random_scene(seed, sizes, m):
    rng = np.random.RandomState(seed)
    levels = [torch.from_numpy(rng.uniform(0, 2, (n, 3)).astype(np.float32)) for n in sizes]
    rows = [_box(*rng.uniform(.3, 1.7, 3), *rng.uniform(.25, 1.4, 3), rng.uniform(-3.5, 3.5) if i % 2 else 0.0) for i in range(m)]
    return levels, rows, rng.randint(0, 18, m).tolist()


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(levels, box rows, labels) -- built once, never modified"""
    if name == "lattice":
        rows = [_box(.48, .48, .48, .64, .64, .64),          # centred on a lattice plane: ties at the k-th centerness
                _box(.40, .44, .45, .30, .30, .30),          # nested in it: the smaller volume wins its rows
                _box(.60, .40, .40, .50, .36, .60, 0.3),     # rotated
                _box(5.0, 5.0, 5.0, .50, .50, .50),          # far from every point: no candidate
                _box(.48, .48, .48, .64, .64, .64)]          # duplicate of the first (another label): equal-volume tie
        return _lattice(), rows, [3, 7, 11, 2, 5]
    if name == "best_level":
        # three levels of 12^3 / 6^3 / 3^3 points: the box over everything has >= 27 on every level (-> the last one), the
        # tiny one < 27 on level 0 (-> -1, clamped to 0), the middle one >= 27 on levels 0 and 1 but not on level 2 (-> 1)
        rows = [_box(.48, .48, .48, 2.0, 2.0, 2.0), _box(.30, .30, .30, .17, .17, .17), _box(.60, .60, .60, .60, .60, .60)]
        return _lattice(((12, .08), (6, .16), (3, .32))), rows, [1, 2, 3]
    if name == "few_points":                                  # n = 7 < topk + 1, on three levels
        pts = _cells(2, .3)[:7]
        return [pts[:4].clone(), pts[4:6].clone(), pts[6:].clone()], [_box(.3, .3, .3, 1.0, 1.0, 1.0)], [4]
    if name == "few_points_one_level":                        # every one of the n = k = 7 rows is a candidate
        return [_cells(2, .3)[:7].clone()], [_box(.31, .27, .34, 1.0, 1.0, 1.0)], [4]
    if name == "awkward":                                     # no size a multiple of 64, level 0 larger than one pass of a workgroup
        return _random_scene(1, (3001, 777, 130, 65), 5)
    if name == "one_box":
        return _random_scene(2, (900, 200, 70, 9), 1)
    if name == "full_capacity":                               # m = m_cap = 16
        return _random_scene(3, (1500, 333, 95, 31), 16)
    raise KeyError(name)


def _ieee_sqrt(x):
    return torch.from_numpy(np.sqrt(x.detach().numpy()))


def _assign_on_cpu(levels, gt, labels):
    with mock.patch.object(torch, "sqrt", _ieee_sqrt):
        return FCAF3DAssigner(LIMIT, TOPK, len(levels)).assign(levels, gt, labels)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """FCAF3DAssigner.assign on the CPU in fp32 -> (centerness [n], box targets [n, 7], labels [n], cs [m, 2], boxes [m, 7])"""
    levels, rows, labels = _scene(name)
    gt = GTBoxes(torch.tensor(rows, dtype=torch.float32))
    ctr, box_t, lab = _assign_on_cpu(levels, gt, torch.tensor(labels))
    ang = -gt.tensor[:, 6]
    return ctr, box_t, lab, torch.stack((torch.cos(ang), torch.sin(ang)), 1), torch.cat((gt.gravity_center, gt.tensor[:, 3:]), 1)


def _run(name, device, m_cap=None):
    levels, rows, labels = _scene(name)
    cs = _reference(name)[3]
    gt = S.DeviceGT.from_boxes(GTBoxes(torch.tensor(rows, dtype=torch.float32)), torch.tensor(labels), device, m_cap=m_cap)
    cs_pad = torch.zeros((gt.boxes.shape[0], 2))
    cs_pad[:len(rows)] = cs
    out = S.assign_targets(torch.cat(levels).to(device), [len(p) for p in levels], gt, LIMIT, TOPK, cs=cs_pad.to(device))
    return gt, [o.cpu() for o in out]


def _check(name, gt, got, n_boxes):
    ctr, box_t, lab, _, boxes = _reference(name)
    labels, pos_row, pos_box, pos_ctr, n_pos = got
    n_pos = int(n_pos)
    assert labels.dtype == torch.int32 and torch.equal(labels.long(), lab.long())
    pos = torch.nonzero(lab >= 0).view(-1)
    assert n_pos == len(pos) <= n_boxes * TOPK
    assert torch.equal(pos_row[:n_pos].long(), pos)                                      # ascending row order
    jb = pos_box[:n_pos].long()
    assert torch.equal(gt.boxes.cpu()[jb].view(torch.int32), box_t[pos].view(torch.int32))          # box target, bit for bit
    assert torch.equal(gt.labels.cpu()[jb], lab[pos].long())                             # the box index (labels tell duplicates apart)
    assert torch.equal(pos_ctr[:n_pos].view(torch.int32), ctr[pos].view(torch.int32))    # centerness target, bit for bit
    assert not pos_row[n_pos:].any() and not pos_box[n_pos:].any() and not pos_ctr[n_pos:].view(torch.int32).any()
    assert pos_row.shape[0] == gt.boxes.shape[0] * TOPK
    return pos, jb


def _level_of(name, rows):
    edges = np.cumsum([len(p) for p in _scene(name)[0]])
    return np.searchsorted(edges, rows.numpy(), side="right")


def test_lattice_scene_ties_nesting_rotation_and_duplicates(device):
    ctr, _, lab, _, _ = _reference("lattice")
    # the premises, on the yardstick: NaN on background rows; box 0 alone keeps fewer than topk rows although it has more
    # candidates (the rows tied at the k-th value all fall to the strict >); three boxes get rows, the duplicate none
    assert torch.isnan(ctr).any()
    levels, rows, _ = _scene("lattice")
    alone = _assign_on_cpu(levels, GTBoxes(torch.tensor(rows[:1])), torch.tensor([3]))[2]
    assert 0 < int((alone >= 0).sum()) < TOPK
    assert sorted(set(lab[lab >= 0].tolist())) == [3, 7, 11]
    gt, got = _run("lattice", device)
    _check("lattice", gt, got, 5)
    gt2, again = _run("lattice", device)
    for a, b in zip(got, again):                              # two calls: identical bytes
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_best_level_branches(device):
    gt, got = _run("best_level", device)
    pos, jb = _check("best_level", gt, got, 3)
    lv = _level_of("best_level", pos)
    for box, level in ((0, 2), (1, 0), (2, 1)):               # last level / -1 clamped to 0 / the middle case
        assert (jb == box).any() and set(lv[(jb == box).numpy()].tolist()) == {level}, (box, level)


@pytest.mark.parametrize("name, expect", [("few_points", 4), ("few_points_one_level", 6)])
def test_fewer_points_than_topk_plus_one(device, name, expect):
    """n = 7: k = min(topk + 1, n) = 7.  Three levels: the 4 rows of level 0 are candidates, the k-th value is a non-candidate's
    -1 and all 4 pass.  One level: all 7 are candidates, the k-th value is the smallest of them and the strict > drops it."""
    gt, got = _run(name, device)
    _check(name, gt, got, 1)
    assert int(got[4]) == expect


@pytest.mark.parametrize("name, m", [("awkward", 5), ("one_box", 1), ("full_capacity", 16)])
def test_awkward_level_sizes_and_box_counts(device, name, m):
    gt, got = _run(name, device)
    assert gt.boxes.shape[0] == 16
    pos, _ = _check(name, gt, got, m)
    assert len(pos) > 0
    if name == "awkward":
        again = _run(name, device)[1]
        for a, b in zip(got, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_one_box_in_a_capacity_of_one(device):
    gt, got = _run("one_box", device, m_cap=1)
    assert gt.boxes.shape[0] == 1 and got[1].shape[0] == TOPK
    _check("one_box", gt, got, 1)


def test_live_counts_below_capacity_equal_the_compact_call(device):
    """NaN and huge values in the dead rows of every level and in the boxes behind m_live: the result is that of the compact call"""
    name = "awkward"
    levels, rows, labels = _scene(name)
    gt_c, compact = _run(name, device)
    pad = (99, 23, 0, 64)
    caps = [len(p) + d for p, d in zip(levels, pad)]
    junk = (float("nan"), 1e30, float("nan"), -1e30)
    padded = torch.cat([torch.cat((p, torch.full((d, 3), j))) for p, d, j in zip(levels, pad, junk)]).to(device)
    live = torch.tensor([len(p) for p in levels], dtype=torch.int32, device=device)
    boxes = gt_c.boxes.clone()
    boxes[len(rows):] = float("nan")
    boxes[len(rows) + 1, :] = 1e30
    lab = gt_c.labels.clone()
    lab[len(rows):] = 1 << 40
    gt = S.DeviceGT(boxes, lab, gt_c.n_live)
    cs = torch.full((16, 2), float("nan"))
    cs[:len(rows)] = _reference(name)[3]
    out = [o.cpu() for o in S.assign_targets(padded, caps, gt, LIMIT, TOPK, level_live=live, cs=cs.to(device))]
    # compact row -> padded row
    shift = torch.cat([torch.full((len(p),), s) for p, s in zip(levels, np.cumsum((0,) + pad[:-1]).tolist())]).long()
    keep = torch.cat([torch.arange(c) < len(p) for p, c in zip(levels, caps)])
    assert torch.equal(out[0][keep], compact[0]) and (out[0][~keep] == -1).all()
    n_pos = int(compact[4])
    assert int(out[4]) == n_pos > 0
    rows_c = compact[1][:n_pos].long()
    assert torch.equal(out[1][:n_pos].long(), rows_c + shift[rows_c])
    assert torch.equal(out[2], compact[2]) and torch.equal(out[3].view(torch.int32), compact[3].view(torch.int32))
    assert not out[1][n_pos:].any()
    _check(name, gt_c, compact, len(rows))


def test_no_boxes(device):
    levels, _, _ = _scene("awkward")
    gt = S.DeviceGT.from_boxes(GTBoxes(torch.zeros((0, 7))), torch.zeros(0, dtype=torch.long), device)
    assert gt.boxes.shape[0] == 16 and int(gt.n_live) == 0
    gt.boxes.fill_(float("nan"))                               # nothing behind m_live = 0 is read
    labels, pos_row, pos_box, pos_ctr, n_pos = S.assign_targets(torch.cat(levels).to(device), [len(p) for p in levels], gt, LIMIT, TOPK)
    assert int(n_pos) == 0 and (labels == -1).all()
    assert not pos_row.any() and not pos_box.any() and not pos_ctr.view(torch.int32).any()
