"""FCAF3DAssigner.assign and the composition of FCAF3DHead.loss (torch path) against the reference's own output, recorded in
tests/golden/fcaf3d_assign.npz by make_golden.py run_assign / run_head_loss: boxes with yaw 0 only (the rotation convention is
third-party and stays unpinned).

Assignment: labels on all rows, box and centerness targets of the positive rows bit for bit, with torch.sqrt replaced by the
correctly rounded one exactly as the fixture's run had it (tests/test_targets_gpu.py says why).

Loss composition: the reference ran with float64 head outputs and float32 points; its three losses were float64 stand-ins that
recorded their arguments.  Here the head's own loss modules are wrapped to record theirs: same labels, same positive rows,
targets and weights bit for bit, n_pos equal, and the three values within 1e-12 relative (float64 evaluations of the same
sums in another order).  One figure of the reference is a float32 sum whose order belongs to the CPU that ran it: the
normaliser of the box loss, max(sum of the positive centerness targets, 1e-6).  The head must hand on exactly that sum of
exactly those targets as this machine computes it; where this machine's sum differs from the recorded one (at most n_pos
float32 roundings) the box loss may differ by that relative amount and no more."""
import pytest
import torch

from targets_fixture import ASSIGN_SCENES, PinnedSqrtAssigner, assign_scene, assigner_on_cpu, load_targets_fixture, loss_scene
from projects.mvsdetection.core.boxes import GTBoxes
from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead


@pytest.fixture(scope="module")
def fixture():
    return load_targets_fixture()


def test_fixture_holds_every_scene_of_the_issue(fixture):
    assert list(fixture["assign.names"]) == ASSIGN_SCENES
    for name in ASSIGN_SCENES:
        sc = assign_scene(fixture, name)
        assert (sc["boxes"][:, 6] == 0).all() and len(set(sc["gt_labels"].tolist())) == len(sc["gt_labels"])
        assert len(sc["labels"]) == sum(len(p) for p in sc["levels"])
        assert len(sc["pos_centerness"]) == int((sc["labels"] >= 0).sum()) > 0
    assert [len(p) for p in assign_scene(fixture, "random")["levels"]] == [3001, 777, 130, 65]
    assert [len(p) for p in assign_scene(fixture, "empty_middle_level")["levels"]] == [900, 0, 70, 9]
    assert assign_scene(fixture, "random_top1_limit1")["limit_topk"].tolist() == [1, 1]
    face = assign_scene(fixture, "point_on_face")
    t = torch.from_numpy(face["levels"][0][64:69])                   # three face points, a corner, one an ulp inside
    assert ((t - 1.0).abs().max(dim=1).values[:4] == 0.5).all() and face["labels"][64:69].tolist() == [-1, -1, -1, -1, 13]


@pytest.mark.parametrize("name", ASSIGN_SCENES)
def test_assigner_equals_the_reference(fixture, name):
    sc = assign_scene(fixture, name)
    ctr, box_t, lab = assigner_on_cpu(sc)
    assert torch.equal(lab.long(), torch.from_numpy(sc["labels"]).long())
    pos = torch.nonzero(lab >= 0).view(-1)
    assert torch.equal(box_t[pos].view(torch.int32), torch.from_numpy(sc["pos_box_target"]).view(torch.int32))
    assert torch.equal(ctr[pos].view(torch.int32), torch.from_numpy(sc["pos_centerness"]).view(torch.int32))


class _Recorder(torch.nn.Module):
    """a loss module of the head, recording the arguments of its one call per scene"""

    def __init__(self, inner, calls):
        super().__init__()
        self.inner, self.calls = inner, calls
        self.loss_weight = inner.loss_weight

    def forward(self, *args, **kw):
        self.calls.append((args, kw))
        return self.inner(*args, **kw)


def test_head_loss_composition_equals_the_reference(fixture):
    scenes = [loss_scene(fixture, s) for s in range(2)]
    head = FCAF3DHead(n_classes=18, in_channels=(8, 8, 8, 8), out_channels=8, n_reg_outs=6, voxel_size=.01, pts_threshold=100000,
                      assigner=dict(type="FCAF3DAssigner", limit=27, topk=18, n_scales=4))
    head.assigner = PinnedSqrtAssigner(head.assigner)
    calls = dict(cls=[], ctr=[], box=[])
    head.loss_cls, head.loss_centerness, head.loss_bbox = (_Recorder(m, calls[k]) for m, k in (
        (head.loss_cls, "cls"), (head.loss_centerness, "ctr"), (head.loss_bbox, "box")))
    per_level = lambda key: [[torch.from_numpy(sc[key][l]).double().requires_grad_(True) for sc in scenes] for l in range(4)]
    loss = head.loss(per_level("centerness"), per_level("bbox_pred"), per_level("cls_score"),
                     [[torch.from_numpy(sc["points"][l]) for sc in scenes] for l in range(4)],
                     [GTBoxes(torch.from_numpy(sc["boxes"])) for sc in scenes],
                     [torch.from_numpy(sc["gt_labels"]).long() for sc in scenes])
    # scene 0 has positive rows, scene 1 none: its centerness and box losses are not called (the reference's else branch)
    assert len(calls["cls"]) == 2 and len(calls["ctr"]) == len(calls["box"]) == 1
    slack = 0.0
    for s, sc in enumerate(scenes):
        h = sc["handed"]
        (score, labels), kw = calls["cls"][s]
        assert torch.equal(labels.long(), torch.from_numpy(h["cls_labels"]).long())                 # which rows are positive
        n_pos = int((h["cls_labels"] >= 0).sum())
        assert float(kw["avg_factor"]) == float(h["cls_avg_factor"]) == max(n_pos, 1)
        assert score.dtype == torch.float64 and score.shape == (len(labels), 18)
        if s == 1:
            assert n_pos == 0
            continue
        (logit, target), kw = calls["ctr"][0]
        assert torch.equal(logit.detach().view(-1), torch.from_numpy(h["ctr_logit"]))
        assert target.dtype == torch.float32 and torch.equal(target.view(-1).view(torch.int32), torch.from_numpy(h["ctr_target"]).view(torch.int32))
        assert float(kw["avg_factor"]) == float(h["ctr_avg_factor"]) == n_pos > 0
        (pred, box_t), kw = calls["box"][0]
        assert torch.equal(pred.detach(), torch.from_numpy(h["box_pred"]))                           # decoded in float64 on both sides
        assert torch.equal(box_t.view(torch.int32), torch.from_numpy(h["box_target"]).view(torch.int32))
        assert torch.equal(kw["weight"].view(torch.int32), torch.from_numpy(h["box_weight"]).view(torch.int32))
        assert torch.equal(kw["weight"], target.view(-1))
        here = max(float(kw["weight"].sum()), 1e-6)                                                  # this machine's float32 sum
        assert float(kw["avg_factor"]) == here
        slack = abs(here - float(h["box_avg_factor"])) / float(h["box_avg_factor"])
        assert slack <= n_pos * 2.0 ** -24
    print(f"relative difference of the float32 normaliser sum between this machine and the fixture's: {slack:.3e}")
    for key in ("loss_centerness", "loss_bbox", "loss_cls"):
        got, exp = float(loss[key].detach()), float(fixture[f"loss.{key}"])
        rel = abs(got - exp) / abs(exp)
        print(f"{key}: {got!r} against the reference's {exp!r}: relative difference {rel:.3e}")
        assert loss[key].dtype == torch.float64 and exp > 0
        assert rel <= 1e-12 + (slack if key == "loss_bbox" else 0.0), key
