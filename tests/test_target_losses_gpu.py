"""The detection losses on the device (cnrma_amd.sparse.focal_loss_sum / positive_loss_sums) and FCAF3DHead(device_targets=True)
against a float64 evaluation of the existing torch modules on the same fp32 inputs; the rotated IoU also against the
polygon-clipping oracle of tests/test_losses_cpu.py.

Tolerance (measured, not fixed): the error of the existing fp32 torch modules against the float64 values is measured on the same
inputs, and the device path may be at most twice that plus one fp32 ulp of the compared quantity (a different but equally valid
evaluation order, another exp / log1p).  Errors are taken in the maximum norm over the compared tensor, the ulp at its largest
magnitude.  Each figure is printed before it is asserted."""
import copy

import numpy as np
import pytest
import torch

from cnrma_amd import sparse as S
from oracle import post_oracle as PO
from projects.mvsdetection.core.boxes import GTBoxes
from projects.mvsdetection.models.fcaf3d_head import (FCAF3DHead, _IoU3DLoss, _SigmoidBCELoss, _SigmoidFocalLoss)

pytestmark = pytest.mark.gpu
TOPK = 18


def _within(what, got, exp64, torch32):
    """|got - exp64| <= 2 |torch32 - exp64| + one fp32 ulp of the quantity (maximum norm)"""
    got, exp64, torch32 = (torch.as_tensor(t).detach().cpu().double().reshape(-1) for t in (got, exp64, torch32))
    assert got.shape == exp64.shape == torch32.shape, what
    if got.numel() == 0:
        return
    assert torch.isfinite(got).all(), what
    e_got, e_ref = float((got - exp64).abs().max()), float((torch32 - exp64).abs().max())
    ulp = float(np.spacing(np.float32(float(exp64.abs().max()))))
    print(f"{what}: device path {e_got:.3e}, fp32 torch modules {e_ref:.3e}, bound {2 * e_ref + ulp:.3e}")
    assert e_got <= 2 * e_ref + ulp, (what, e_got, e_ref, ulp)


# ---- focal loss -------------------------------------------------------------------------------------------------------------------
def _focal_inputs(n_cls, background_only=False):
    rng = np.random.RandomState(n_cls)
    caps, live = (150, 40, 13, 5), (131, 40, 0, 4)                  # a level with dead rows, a full one, an empty one
    n = sum(caps)
    x = (rng.randn(n, n_cls) * 4).astype(np.float32)
    x[rng.rand(n, n_cls) < 0.05] = 30.0
    x[rng.rand(n, n_cls) < 0.05] = -30.0
    labels = np.full(n, -1, dtype=np.int32)
    if not background_only:
        hit = rng.rand(n) < 0.2
        labels[hit] = rng.randint(0, n_cls, hit.sum())
        labels[5], labels[6] = n_cls, 0                             # outside [0, n_cls): a background row; class 0
        x[6, 0], x[7, 1] = 30.0, -30.0
        labels[7] = 1
    keep = np.concatenate([np.arange(c) < l for c, l in zip(caps, live)])
    x[~keep] = np.nan                                               # dead rows hold anything
    labels[~keep] = 3
    return caps, live, torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(keep)


def _focal_reference(x, labels, dtype):
    p = x.to(dtype).requires_grad_(True)
    loss = _SigmoidFocalLoss(gamma=2.0, alpha=0.25)(p, labels.long(), avg_factor=1.0)
    return loss.detach(), torch.autograd.grad(loss, p)[0]


@pytest.mark.parametrize("n_cls, background_only", [(18, False), (17, False), (18, True)])
def test_focal_loss_and_gradient(device, n_cls, background_only):
    caps, live, x, labels, keep = _focal_inputs(n_cls, background_only)
    exp, g_exp = _focal_reference(x[keep], labels[keep], torch.float64)
    t32, g_t32 = _focal_reference(x[keep], labels[keep], torch.float32)
    xd = x.to(device).requires_grad_(True)
    out = S.focal_loss_sum(xd, labels.to(device), caps, torch.tensor(live, dtype=torch.int32, device=device), 2.0, 0.25)
    (g,) = torch.autograd.grad(out * 0.5, xd)                      # backward multiplies by the incoming scalar
    assert out.dtype == torch.float32 and out.dim() == 0
    _within("focal sum", out, exp, t32)
    _within("focal gradient", g.cpu()[keep] * 2, g_exp, g_t32)
    assert not g.cpu()[~keep].view(torch.int32).any()               # zeros on dead rows, whatever they hold
    again = S.focal_loss_sum(xd, labels.to(device), caps, torch.tensor(live, dtype=torch.int32, device=device), 2.0, 0.25)
    assert torch.equal(out.detach(), again.detach())


# ---- positive rows ----------------------------------------------------------------------------------------------------------------
def _gt(rng, m, yaw):
    b = np.zeros((16, 7), dtype=np.float32)
    b[:m, :3] = rng.randn(m, 3) * 0.6
    b[:m, 3:6] = 0.3 + rng.rand(m, 3) * 1.5
    if yaw:
        b[:m, 6] = rng.uniform(-np.pi, np.pi, m)
        b[0, 6], b[1, 6] = 4.0, -5.5                               # wrapped yaws
    b[m:] = np.nan
    return b


def _positive_inputs(rotated, n_pos, seed=0):
    rng = np.random.RandomState(seed)
    m, p_cap = 9, 16 * TOPK
    gt = _gt(rng, m, rotated)
    pos_box = np.zeros(p_cap, dtype=np.int32)
    pos_box[:n_pos] = rng.randint(0, m, n_pos)
    pos_ctr = np.zeros(p_cap, dtype=np.float32)
    pos_ctr[:n_pos] = rng.rand(n_pos)
    pred = np.full((p_cap, 7 if rotated else 6), np.nan, dtype=np.float32)      # dead rows hold anything
    t = gt[pos_box[:n_pos]]
    pred[:n_pos, :3] = t[:, :3] + rng.randn(n_pos, 3) * 0.25
    pred[:n_pos, 3:6] = t[:, 3:6] * rng.uniform(0.6, 1.5, (n_pos, 3))
    if rotated:
        pred[:n_pos, 6] = t[:, 6] + rng.randn(n_pos) * 0.5
        pred[:4, 6] += 2 * np.pi                                    # |yaw| > pi on the predicted side too
    logit = np.full(p_cap, np.nan, dtype=np.float32)
    logit[:n_pos] = rng.randn(n_pos) * 3
    logit[:2] = (30.0, -30.0)
    return tuple(torch.from_numpy(a) for a in (gt, pos_box, pos_ctr, pred, logit))


def _positive_reference(gt, pos_box, pos_ctr, pred, logit, n_pos, rotated, dtype):
    x, b = logit[:n_pos].to(dtype).requires_grad_(True), pred[:n_pos].to(dtype).requires_grad_(True)
    w = pos_ctr[:n_pos].to(dtype)
    bce = _SigmoidBCELoss()(x[:, None], w[:, None], avg_factor=1.0)
    iou = _IoU3DLoss(with_yaw=rotated)(b, gt[pos_box[:n_pos].long()].to(dtype), weight=w, avg_factor=1.0)
    gx, gb = torch.autograd.grad(bce + iou, (x, b))
    return bce.detach(), iou.detach(), w.sum(), gx, gb


def _positive_device(device, gt, pos_box, pos_ctr, pred, logit, n_pos, rotated):
    g = S.DeviceGT(gt.to(device), torch.zeros(16, dtype=torch.int64, device=device), torch.full((1,), 9, dtype=torch.int32, device=device))
    x, b = logit.to(device).requires_grad_(True), pred.to(device).requires_grad_(True)
    sums = S.positive_loss_sums(x, b, g, pos_box.to(device), pos_ctr.to(device),
                                torch.full((1,), n_pos, dtype=torch.int32, device=device), rotated)
    gx, gb = torch.autograd.grad(sums[0] + sums[1], (x, b))
    return sums.detach().cpu(), gx.cpu(), gb.cpu()


@pytest.mark.parametrize("rotated", [False, True])
def test_positive_row_losses_and_gradients(device, rotated):
    n_pos = 150
    inp = _positive_inputs(rotated, n_pos)
    exp = _positive_reference(*inp, n_pos, rotated, torch.float64)
    t32 = _positive_reference(*inp, n_pos, rotated, torch.float32)
    sums, gx, gb = _positive_device(device, *inp, n_pos, rotated)
    for i, what in enumerate(("centerness BCE sum", "IoU loss sum", "sum of centerness targets")):
        _within(what, sums[i], exp[i], t32[i])
    _within("centerness gradient", gx[:n_pos], exp[3], t32[3])
    _within("box gradient", gb[:n_pos], exp[4], t32[4])
    assert float(exp[4].abs().max()) > 1e-3 and (not rotated or float(exp[4][:, 6].abs().max()) > 1e-3)
    assert not gx[n_pos:].view(torch.int32).any() and not gb[n_pos:].view(torch.int32).any()      # dead rows: zero gradients
    if rotated:                                                     # the polygon-clipping oracle, with unit weights
        gt, pos_box, pos_ctr, pred, logit = inp
        ones = torch.zeros_like(pos_ctr)
        ones[:n_pos] = 1.0
        got = _positive_device(device, gt, pos_box, ones, pred, logit, n_pos, True)[0][1]
        orc = sum(1.0 - PO.iou(a, b, mode3d=True) for a, b in zip(pred[:n_pos].double().numpy(), gt[pos_box[:n_pos].long()].double().numpy()))
        print(f"IoU loss sum against the clipping oracle: {abs(float(got) - orc):.3e}")
        assert abs(float(got) - orc) <= float(np.spacing(np.float32(orc))) + 1e-9 * n_pos


@pytest.mark.parametrize("rotated", [False, True])
def test_iou_special_cases_by_value(device, rotated):
    """identical, disjoint, contained, edge-touching: values only (the reference's gradients are arbitrary there)"""
    cols = 7 if rotated else 6
    yaw = 0.4 if rotated else 0.0
    base = np.array([0.2, -0.1, 0.3, 1.0, 0.8, 0.6, yaw], dtype=np.float32)
    gt = np.full((16, 7), np.nan, dtype=np.float32)
    gt[:4] = base
    pred = np.tile(base, (4, 1))
    pred[1, :3] += 50.0                                             # disjoint
    pred[2, 3:6] *= 0.4                                             # contained
    c, s = np.cos(np.float32(yaw)), np.sin(np.float32(yaw))
    pred[3, 0] += base[3] * c                                       # shares a face: shifted by its own length along its x axis
    pred[3, 1] += base[3] * s
    p_cap = 16 * TOPK
    pad = lambda a, fill: torch.from_numpy(np.concatenate((a, np.full((p_cap - len(a),) + a.shape[1:], fill, dtype=a.dtype))))
    inp = (torch.from_numpy(gt), pad(np.arange(4, dtype=np.int32), 0), pad(np.ones(4, dtype=np.float32), 0.0),
           pad(pred[:, :cols].copy(), np.nan), pad(np.zeros(4, dtype=np.float32), np.nan))
    for k in range(4):                                              # one row at a time: the sum is that row's 1 - IoU
        one = (inp[0], inp[1][k:].contiguous()[:p_cap - 4], inp[2][k:].contiguous()[:p_cap - 4], inp[3][k:].contiguous()[:p_cap - 4],
               inp[4][k:].contiguous()[:p_cap - 4])
        exp = _positive_reference(*one, 1, rotated, torch.float64)[1]
        t32 = _positive_reference(*one, 1, rotated, torch.float32)[1]
        g = S.DeviceGT(one[0].to(device), torch.zeros(16, dtype=torch.int64, device=device), torch.full((1,), 4, dtype=torch.int32, device=device))
        sums = S.positive_loss_sums(one[4].to(device), one[3].to(device), g, one[1].to(device), one[2].to(device),
                                    torch.ones(1, dtype=torch.int32, device=device), rotated)
        _within(f"1 - IoU of special case {k}", sums[1], exp, t32)
    assert abs(float(exp) - 1.0) < 1e-6                             # the last one: touching boxes share no volume


@pytest.mark.parametrize("rotated", [False, True])
def test_no_positive_rows(device, rotated):
    inp = _positive_inputs(rotated, 0)
    sums, gx, gb = _positive_device(device, *inp, 0, rotated)
    assert not sums.view(torch.int32).any() and not gx.view(torch.int32).any() and not gb.view(torch.int32).any()


# ---- the head -----------------------------------------------------------------------------------------------------------------------
def _cells(n, step):
    g = (torch.arange(n, dtype=torch.float32) + 0.5) * step
    return torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()


def _head(arkit, device_targets):
    torch.manual_seed(0)
    kw = dict(n_reg_outs=8, yaw_parametrization="fcaf3d", loss_bbox=dict(type="IoU3DLoss", with_yaw=True, loss_weight=1.0)) if arkit \
        else dict(n_reg_outs=6)
    return FCAF3DHead(n_classes=18, in_channels=(8, 8, 8, 8), out_channels=8, voxel_size=.01, pts_threshold=100000,
                      assigner=dict(type="FCAF3DAssigner", limit=27, topk=TOPK, n_scales=4), device_targets=device_targets, **kw)


def _gt_rows(arkit, m, seed):
    rng = np.random.RandomState(seed)
    rows = np.zeros((m, 7), dtype=np.float32)
    rows[:, 3:6] = rng.uniform(.2, .7, (m, 3))
    rows[:, :3] = rng.uniform(.2, .8, (m, 3))
    rows[:, 2] -= rows[:, 5] / 2
    if arkit:
        rows[:, 6] = rng.uniform(-3.0, 3.0, m)
    return torch.from_numpy(rows), torch.from_numpy(rng.randint(0, 18, m))


def _head_outputs(arkit, seed=0):
    """a four-level scene (12^3 / 6^3 / 3^3 / 2^3 cell centres): per level one scene's centerness, box, class outputs and points"""
    rng = np.random.RandomState(seed)
    pts = [_cells(n, s) for n, s in ((12, .08), (6, .16), (3, .32), (2, .64))]
    cen = [torch.from_numpy(rng.randn(len(p), 1).astype(np.float32)) for p in pts]
    box = [torch.from_numpy(np.concatenate((rng.uniform(.05, .45, (len(p), 6)), rng.randn(len(p), 2) if arkit else np.zeros((len(p), 0))),
                                           axis=1).astype(np.float32)) for p in pts]
    cls = [torch.from_numpy((rng.randn(len(p), 18) * 2 - 3).astype(np.float32)) for p in pts]
    return cen, box, cls, pts


class _Fp64Targets:
    """the assigner's fp32 decisions and targets, handed on as float64: the float64 evaluation starts from the same targets"""

    def __init__(self, inner):
        self.inner, self.limit, self.topk, self.n_scales = inner, inner.limit, inner.topk, inner.n_scales

    def assign(self, points, gt_bboxes, gt_labels):
        c, b, l = self.inner.assign([p.float() for p in points], gt_bboxes, gt_labels)
        return c.double(), b.double(), l


def _head_loss(head, outs, gt_boxes, gt_labels, device, dtype=torch.float32):
    cen, box, cls, pts = outs
    leaves = [[t.to(device=device, dtype=dtype).requires_grad_(True) for t in group] for group in (cen, box, cls)]
    loss = head.loss(*[[[t] for t in group] for group in leaves], [[p.to(device)] for p in pts], [gt_boxes], [gt_labels])
    names = ("loss_centerness", "loss_bbox", "loss_cls")
    grads = torch.autograd.grad(sum(loss[k] for k in names), [t for group in leaves for t in group])
    return [loss[k].detach() for k in names], [torch.cat(grads[4 * i:4 * i + 4]) for i in range(3)]


@pytest.mark.parametrize("arkit", [False, True])
def test_head_loss_equals_the_torch_path(device, arkit):
    outs = _head_outputs(arkit)
    rows, labels = _gt_rows(arkit, 5, seed=1)
    cpu = torch.device("cpu")
    t32 = _head_loss(_head(arkit, False), outs, GTBoxes(rows), labels, cpu)
    ref = _head(arkit, False)
    ref.assigner = _Fp64Targets(ref.assigner)
    exp = _head_loss(ref, outs, GTBoxes(rows), labels, cpu, torch.float64)
    got = _head_loss(_head(arkit, True), outs, GTBoxes(rows).to(device), labels.to(device), device)
    assert float(exp[0][1]) > 0 and float(exp[1][1].abs().max()) > 0          # there are positive rows
    for i, what in enumerate(("loss_centerness", "loss_bbox", "loss_cls")):
        _within(what, got[0][i], exp[0][i], t32[0][i])
    for i, what in enumerate(("centerness", "bbox_pred", "cls_score")):
        _within(f"gradient of {what}", got[1][i], exp[1][i], t32[1][i])


def test_head_loss_without_boxes(device):
    """no ground-truth box: centerness and box losses are zero with zero gradients, the focal loss runs over background rows"""
    outs = _head_outputs(False)
    got = _head_loss(_head(False, True), outs, GTBoxes(torch.zeros((0, 7))).to(device), torch.zeros(0, dtype=torch.long, device=device), device)
    assert float(got[0][0]) == 0 and float(got[0][1]) == 0 and float(got[0][2]) > 0
    assert not got[1][0].any() and not got[1][1].any() and got[1][2].abs().max() > 0
    x = torch.cat(outs[2])
    exp = _focal_reference(x, torch.full((len(x),), -1), torch.float64)
    t32 = _focal_reference(x, torch.full((len(x),), -1), torch.float32)
    _within("background-only loss_cls", got[0][2], exp[0], t32[0])


def test_no_host_read_under_loss_and_backward(device):
    outs = _head_outputs(False)
    rows, labels = _gt_rows(False, 5, seed=1)
    gt, labels = GTBoxes(rows).to(device), labels.to(device)
    on, off = _head(False, True), _head(False, False)
    _head_loss(on, outs, gt, labels, device)                       # warm-up: library load, allocator
    leaves = [[t.to(device).requires_grad_(True) for t in group] for group in outs[:3]]
    pts = [[p.to(device)] for p in outs[3]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = on.loss(*[[[t] for t in group] for group in leaves], pts, [gt], [labels])
        (loss["loss_centerness"] + loss["loss_bbox"] + loss["loss_cls"]).backward()
        with pytest.raises(RuntimeError):                           # the check bites: the torch path reads the device back
            off.loss(*[[[t] for t in group] for group in leaves], pts, [gt], [labels])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for group in leaves for t in group)


@pytest.mark.parametrize("arkit", [False, True])
def test_loss_and_backward_in_a_graph(device, arkit):
    """loss + backward from leaf copies of the head outputs, captured once; replayed on other ground truth (3 and 11 boxes inside
    m_cap = 16) by copying into the DeviceGT buffers: every replay equals the eager device path bit for bit"""
    head = _head(arkit, True)
    outs = _head_outputs(arkit)
    leaves = [[t.to(device).requires_grad_(True) for t in group] for group in outs[:3]]
    flat = [t for group in leaves for t in group]
    pts = [[p.to(device)] for p in outs[3]]
    truths = [S.DeviceGT.from_boxes(GTBoxes(r), l, device, m_cap=16) for r, l in (_gt_rows(arkit, 3, seed=2), _gt_rows(arkit, 11, seed=3))]
    static = S.DeviceGT(torch.zeros((16, 7), device=device), torch.zeros(16, dtype=torch.int64, device=device),
                        torch.zeros(1, dtype=torch.int32, device=device))

    def load(src):
        static.boxes.copy_(src.boxes), static.labels.copy_(src.labels), static.n_live.copy_(src.n_live)

    def run(gt):
        loss = head.loss(*[[[t] for t in group] for group in leaves], pts, [gt], [None])
        names = ("loss_centerness", "loss_bbox", "loss_cls")
        return [loss[k] for k in names] + list(torch.autograd.grad(sum(loss[k] for k in names), flat))

    eager = [[t.detach().clone() for t in run(gt)] for gt in truths]
    assert float(eager[0][1]) > 0 and float(eager[1][1]) > 0 and not torch.equal(eager[0][1], eager[1][1])
    load(truths[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outputs = run(static)
    for which in (1, 0):
        load(truths[which])
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip(outputs, eager[which]):
            assert torch.equal(got.detach(), exp)
