"""Readers of tests/golden/fcaf3d_assign.npz (make_golden.py run_assign / run_head_loss): what the reference's FCAF3DAssigner
and FCAF3DHead.loss gave on scenes of yaw-0 boxes, shared by the CPU and the GPU tests of the targets."""
import os
from unittest import mock

import numpy as np
import torch

from helpers import GOLDEN

ASSIGN_SCENES = ["lattice", "best_level", "few_points", "few_points_one_level", "random", "random_top1_limit1",
                 "empty_middle_level", "point_on_face"]


def load_targets_fixture():
    z = np.load(os.path.join(GOLDEN, "fcaf3d_assign.npz"))
    return {k: z[k] for k in z.files}


def assign_scene(fixture, name):
    """levels (list of [n_i, 3]), boxes [m, 7] = (x, y, z_bottom, dx, dy, dz, 0), gt_labels, limit_topk and the reference's labels
    [n] (int16), pos_box_target [P, 7], pos_centerness [P] (the rows with label >= 0, ascending)"""
    pre = f"assign.{name}."
    sc = {k[len(pre):]: v for k, v in fixture.items() if k.startswith(pre)}
    sc["levels"] = [sc.pop(f"level{i}") for i in range(sum(k.startswith("level") for k in sc))]
    return sc


def loss_scene(fixture, s):
    """per level: points, centerness, bbox_pred, cls_score; boxes, gt_labels; handed = what the reference gave its three losses"""
    pre = f"loss.scene{s}."
    sc = {k[len(pre):]: v for k, v in fixture.items() if k.startswith(pre)}
    out = dict(boxes=sc["boxes"], gt_labels=sc["gt_labels"],
               handed={k[len("handed."):]: v for k, v in sc.items() if k.startswith("handed.")})
    for key in ("points", "centerness", "bbox_pred", "cls_score"):
        out[key] = [sc[f"{key}{l}"] for l in range(4)]
    return out


def ieee_sqrt(x):
    """the correctly rounded square root, for torch.sqrt on the CPU (tests/test_targets_gpu.py says why)"""
    with np.errstate(invalid="ignore"):                        # background rows hold NaN, as in torch
        return torch.from_numpy(np.sqrt(x.detach().numpy()))


def assign_on_cpu(levels, gt, labels, limit, topk):
    """this repository's FCAF3DAssigner.assign in float32 on the CPU with the pinned square root -> (centerness, box targets, labels)"""
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DAssigner
    with mock.patch.object(torch, "sqrt", ieee_sqrt):
        return FCAF3DAssigner(limit, topk, len(levels)).assign(levels, gt, labels)


def assigner_on_cpu(sc):
    from projects.mvsdetection.core.boxes import GTBoxes
    limit, topk = (int(v) for v in sc["limit_topk"])
    return assign_on_cpu([torch.from_numpy(p) for p in sc["levels"]], GTBoxes(torch.from_numpy(sc["boxes"])),
                         torch.from_numpy(sc["gt_labels"]).long(), limit, topk)


class PinnedSqrtAssigner:
    """an FCAF3DAssigner run with the pinned square root, for a head's `assigner`"""

    def __init__(self, inner):
        self.inner, self.limit, self.topk, self.n_scales = inner, inner.limit, inner.topk, inner.n_scales

    def assign(self, points, gt_bboxes, gt_labels):
        with mock.patch.object(torch, "sqrt", ieee_sqrt):
            return self.inner.assign(points, gt_bboxes, gt_labels)
